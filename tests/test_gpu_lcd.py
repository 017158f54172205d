"""GPU parity: DeepLCD/CALC descriptor (f32, stated tolerance) and the loop-database scan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# f32 network, different summation order on the GPU (MFMA k-order, wave reductions) and powf implementations:
# descriptor entries are O(0.03) after normalisation; 2e-5 absolute is ~1e-3 relative of a typical entry.
DESC_ATOL = 2e-5
SCORE_ATOL = 2e-5


def _nhwc_to_nchw(a, h, w, c):
    return a.reshape(h, w, c).transpose(2, 0, 1)


def test_preproc_and_descriptor(api, oracle, synth):
    w = synth.calc_weights()
    lcd = api.DeepLCD(w)
    for sid in (0, 1):
        L, _ = synth.stereo_pair(sid, 2)
        d, after = lcd.calcDescrOriginalImg(L, blur_in_place=True)
        x, rafter = oracle.calc_preproc(L, blur_in_place=True)
        assert np.array_equal(after, rafter), "in-place 7x7 blur (deeplcd.cpp:46) must be bit-exact"
        ref = oracle.calc_forward(w, x)
        assert np.abs(d - ref).max() < DESC_ATOL, np.abs(d - ref).max()
        assert abs(np.linalg.norm(d) - 1) < 1e-5
        d2, after2 = lcd.calcDescrOriginalImg(L, blur_in_place=False)
        assert np.array_equal(after2, L) and np.array_equal(d, d2)
        small = oracle.resize(oracle.blur7(L, 1), 160, 120)
        d3 = lcd.calcDescr(small)                                   # DeepLCD::calcDescr on the already-resized image
        assert np.abs(d3 - ref).max() < DESC_ATOL


def test_layer_taps_against_torch(api, synth):
    """Stage taps 0 .. 3 and the descriptor against the f64 net (tests/calc_f64.py: CPU torch, double precision), both kernel families."""
    import calc_f64
    w = synth.calc_weights()
    x = synth._rng(21).uniform(0, 1, (120, 160)).astype(np.float32)
    refs = calc_f64.forward_f64(calc_f64.default_layers(), w, x)
    assert [r.shape for r in refs] == [(64, 62, 82), (64, 31, 41), (128, 32, 42), (128, 16, 21), (1064,)]
    lcd = api.DeepLCD(w)
    lcd2 = api.DeepLCD(w); lcd2.set_option(lcd2.OPT_CONV2_BF16X6, 1)            # the bf16 x 6 fallback kernels hold the same bar
    assert lcd.conv2_products() == 3 and lcd2.conv2_products() == 6
    for family, h in (("f16x3", lcd), ("bf16x6", lcd2)):
        for stage in range(4):
            ref = refs[stage]
            got = calc_f64.nhwc_to_nchw(h.debug_forward(x, stage), ref.shape)
            err = np.abs(got - ref).max() / max(1e-6, np.abs(ref).max())
            # f32-level accuracy is what the f16 x 3 / bf16 x 6 split products on the 16-bit matrix cores claim (measured 1.1e-6 against this
            # f64 net, tools/conv2_error.py): the bar is 5e-6 max-normalised, not the 2e-5 ABSOLUTE bar against the f32 oracle (an asymmetric
            # weight bank: a transposed tile would fail here by orders of magnitude)
            assert err < 5e-6, (family, stage, err)
        assert np.abs(h.debug_forward(x, 4) - refs[4]).max() < DESC_ATOL, family


def test_describe_batch(api, oracle, synth):
    import torch
    w = synth.calc_weights(); lcd = api.DeepLCD(w)
    B = 5
    imgs = np.stack([synth.stereo_pair(0, t)[0] for t in range(B)])
    d_imgs = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    assert d_imgs.is_contiguous(); d_out = torch.zeros(B, 1064, device="cuda")
    lcd.describe_batch(d_imgs.data_ptr(), B, 376, 1241, 1241, 376 * 1241, d_out.data_ptr(), blur_in_place=False)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(d_imgs.cpu().numpy(), imgs)
    for b in range(B):
        x, _ = oracle.calc_preproc(imgs[b])
        assert np.abs(out[b] - oracle.calc_forward(w, x)).max() < DESC_ATOL
    lcd.describe_batch(d_imgs.data_ptr(), B, 376, 1241, 1241, 376 * 1241, d_out.data_ptr(), blur_in_place=True)
    torch.cuda.synchronize()
    assert np.array_equal(d_imgs.cpu().numpy()[2], oracle.blur7(imgs[2], 1))
    assert np.abs(d_out.cpu().numpy() - out).max() == 0


def test_score(api, oracle, synth):
    db = synth.lcd_database(4)
    assert api.DeepLCD.score(db[0], db[1]) == pytest.approx(oracle.lcd_score(db[0], db[1]), abs=1e-6)
    assert api.DeepLCD.score(db[2], db[2]) == pytest.approx(1.0, abs=1e-5)


@pytest.mark.parametrize("n", [60, 1000, 10000])
def test_loop_database_scan(api, oracle, synth, n):
    db = synth.lcd_database(n)
    ids = (np.arange(n, dtype=np.uint64) * 3 + 5)
    D = api.LoopDatabase(n + 7)
    for i in range(min(n, 40)):
        D.AddToDatabase(int(ids[i]), db[i])                          # one-by-one like LoopClosing::AddToDatabase
    if n > 40:
        import torch
        t = torch.from_numpy(db[40:]).cuda()
        D.append_batch(ids[40:], t.data_ptr(), n - 40)
    assert len(D) == n
    rng = np.random.default_rng(n)
    for trial in range(6):
        q = db[rng.integers(0, n)] * 0.97 + 0.03 * synth.lcd_database(1, seed=trial + 1)[0]
        q = (q / np.linalg.norm(q)).astype(np.float32)
        cur = int(ids[-1] + 20) if trial < 3 else int(ids[rng.integers(n // 2, n)])
        best, mx, cnt = D.query(q, cur)
        rbest, rmx, rcnt = oracle.lcddb_query(db, ids, q, cur)
        assert best == rbest and abs(mx - rmx) < SCORE_ATOL
        scores = db @ q
        near = np.abs(scores - 0.92) < 1e-5                          # counts may only differ for scores within float noise of the threshold
        assert abs(cnt - rcnt) <= int(near.sum())
    with pytest.raises(api.MyslamError):
        D.AddToDatabase(int(ids[-1]), db[0])                         # ids must ascend (std::map order)


def test_loop_database_grows_like_the_std_map(api, oracle, synth):
    """LoopClosing::_mvDatabase is an unbounded std::map (loopclosing.h:120, loopclosing.cpp:651-659): AddToDatabase must never fail for
    lack of room.  A handle created for 8 key-frames takes 700 one by one and a 2 000-row device batch; every scan equals the oracle's."""
    import torch
    n1, n2 = 700, 2000
    db = synth.lcd_database(n1 + n2); ids = np.arange(n1 + n2, dtype=np.uint64) * 2 + 1
    D = api.LoopDatabase(8)
    cap0 = D.capacity()
    grown = 0
    for i in range(n1):
        D.AddToDatabase(int(ids[i]), db[i])
        if D.capacity() != cap0:
            grown += 1; cap0 = D.capacity()
        if i in (7, 8, 63, 64, 65, 300, n1 - 1):                      # straight after a move and between moves
            got = D.query(db[i // 2], int(ids[i]) + 20); ref = oracle.lcddb_query(db[:i + 1], ids[:i + 1], db[i // 2], int(ids[i]) + 20)
            assert got[0] == ref[0] and abs(got[1] - ref[1]) < SCORE_ATOL and got[2] == ref[2], i
    assert len(D) == n1 and grown >= 3 and D.capacity() >= n1
    t = torch.from_numpy(db[n1:]).cuda()
    D.append_batch(ids[n1:], t.data_ptr(), n2)                        # one batch larger than twice the capacity
    assert len(D) == n1 + n2 and D.capacity() >= n1 + n2
    D.reserve(10000); c = D.capacity(); assert c >= 10000
    D.reserve(100); assert D.capacity() == c                          # never shrinks
    nq = 64
    qs = db[np.random.default_rng(5).integers(0, n1 + n2, nq)].copy()
    cur = np.full(nq, int(ids[-1]) + 20, np.uint64); cur[::3] = ids[n1 + 5]
    d_q = torch.from_numpy(qs).cuda()
    d_best = torch.zeros(nq, dtype=torch.int64, device="cuda"); d_max = torch.zeros(nq, device="cuda"); d_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    D.query_batch(d_q.data_ptr(), cur, nq, d_best.data_ptr(), d_max.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    for i in range(nq):
        ref = oracle.lcddb_query(db, ids, qs[i], int(cur[i]))
        assert int(d_best[i]) == ref[0] and abs(float(d_max[i]) - ref[1]) < SCORE_ATOL and int(d_cnt[i]) == ref[2], i


def test_loop_database_rules(api, oracle, synth):
    db = synth.lcd_database(100); ids = np.arange(100, dtype=np.uint64) * 2
    D = api.LoopDatabase(100)
    for i in range(100):
        D.AddToDatabase(int(ids[i]), db[i])
    db2 = db.copy()
    assert D.query(db[37], 300)[0] == 74
    assert D.query(db[37], 5) == (0, 0.0, 0)                         # nothing older than 20 ids -> bestId 0, maxScore 0
    for cur in (19, 20, 21, 39, 40, 41, 90, 197, 198, 199, 218, 219):
        got = D.query(db[10], cur); ref = oracle.lcddb_query(db2, ids, db[10], cur)
        assert got[0] == ref[0] and abs(got[1] - ref[1]) < SCORE_ATOL and got[2] == ref[2], cur
    ok, cand = D.DetectLoop(db[37], 300)
    assert ok and cand == 74
    assert D.DetectLoop(synth.lcd_database(1, seed=5)[0], 300) == (False, None)


def test_loop_database_batch_queries(api, oracle, synth):
    import torch
    n, nq = 3000, 37
    db = synth.lcd_database(n); ids = np.arange(n, dtype=np.uint64)
    D = api.LoopDatabase(n)
    t = torch.from_numpy(db).cuda(); D.append_batch(ids, t.data_ptr(), n)
    rng = np.random.default_rng(8)
    q = db[rng.integers(0, n, nq)] * 0.9 + 0.1 * synth.lcd_database(nq, seed=77)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    cur = rng.integers(100, n + 40, nq).astype(np.uint64)
    dq = torch.from_numpy(q).cuda()
    dbest = torch.zeros(nq, dtype=torch.int64, device="cuda"); dmax = torch.zeros(nq, device="cuda"); dcnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    D.query_batch(dq.data_ptr(), cur, nq, dbest.data_ptr(), dmax.data_ptr(), dcnt.data_ptr())
    torch.cuda.synchronize()
    for i in range(nq):
        rb, rm, rc = oracle.lcddb_query(db, ids, q[i], int(cur[i]))
        assert int(dbest[i]) == rb and abs(float(dmax[i]) - rm) < SCORE_ATOL and int(dcnt[i]) == rc


def test_loop_database_many_queries_back_to_back(api, oracle, synth):
    """2048 queries per call (what an 8-GPU run sends to every shard: 256 frames x 8 ranks), issued twice without a host
    synchronisation in between (the per-query row limits travel through a pinned buffer)."""
    import torch
    n, nq = 700, 2048
    db = synth.lcd_database(n); ids = np.arange(0, 2 * n, 2, dtype=np.uint64)
    D = api.LoopDatabase(n)
    t = torch.from_numpy(db).cuda(); D.append_batch(ids, t.data_ptr(), n)
    rng = np.random.default_rng(9)
    outs = []
    for rep in range(2):
        q = db[rng.integers(0, n, nq)] * 0.9 + 0.1 * synth.lcd_database(nq, seed=78 + rep)
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        cur = rng.integers(50, 2 * n + 60, nq).astype(np.uint64)
        dq = torch.from_numpy(q).cuda()
        dbest = torch.zeros(nq, dtype=torch.int64, device="cuda"); dmax = torch.zeros(nq, device="cuda"); dcnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        D.query_batch(dq.data_ptr(), cur, nq, dbest.data_ptr(), dmax.data_ptr(), dcnt.data_ptr())
        outs.append((q, cur, dq, dbest, dmax, dcnt))
    torch.cuda.synchronize()
    for q, cur, _, dbest, dmax, dcnt in outs:
        for i in range(0, nq, 37):
            rb, rm, rc = oracle.lcddb_query(db, ids, q[i], int(cur[i]))
            assert int(dbest[i]) == rb and abs(float(dmax[i]) - rm) < SCORE_ATOL and int(dcnt[i]) == rc


def _db_check(oracle, db, ids, q, cur, dbest, dmax, dcnt, rows):
    """device results of queries `rows` against the oracle's scan (the oracle scan costs ~n x 1064 flops per query on one core)"""
    for i in rows:
        rb, rm, rc = oracle.lcddb_query(db, ids, q[i], int(cur[i]))
        scores = db @ q[i]
        near = int((np.abs(scores - 0.92) < 1e-5).sum())                 # counts may only differ for scores within float noise of the threshold
        assert int(dbest[i]) == rb and abs(float(dmax[i]) - rm) < SCORE_ATOL and abs(int(dcnt[i]) - rc) <= near, i


def test_loop_database_configs4_shard_shape(api, oracle, synth):
    """BASELINE configs[4] per GPU: a 6 250-row shard of the 50 000-KF database scored against 4 096 queries per call (512 frames x
    8 ranks), through the sharded entry point; 128 of the queries are checked against the oracle's scan, all of them against an f64
    matrix product; the break flag of every record against the id rule."""
    import torch
    n, nq, shard = 6250, 4096, 3
    db = synth.lcd_database(n, seed=0xDB + shard); ids = np.arange(shard * n, (shard + 1) * n, dtype=np.uint64)
    D = api.LoopDatabase(n)
    t = torch.from_numpy(db).cuda(); D.append_batch(ids, t.data_ptr(), n)
    rng = np.random.default_rng(44)
    q = db[rng.integers(0, n, nq)] * 0.85 + 0.15 * synth.lcd_database(nq, seed=79)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    cur = np.full(nq, 8 * n + 20, np.uint64)
    cur[::5] = rng.integers(shard * n - 50, (shard + 1) * n + 50, len(cur[::5])).astype(np.uint64)      # some scans stop inside / before / after this shard
    dq = torch.from_numpy(q).cuda()
    cand = torch.zeros(nq * 16, dtype=torch.uint8, device="cuda")
    D.query_batch_sharded(dq.data_ptr(), cur, nq, cand.data_ptr())
    torch.cuda.synchronize()
    rec = cand.cpu().numpy().view(api.CAND_DTYPE)
    broke = rec["cnt"] < 0
    assert np.array_equal(broke, pkg_breaks(ids, cur))
    cnt = rec["cnt"] & 0x7fffffff
    _db_check(oracle, db, ids, q, cur, rec["best_id"], rec["max_score"], cnt, range(0, nq, 32))
    # every query: scores of the rows the scan may see, in f64
    S = db.astype(np.float64) @ q.astype(np.float64).T                  # [n, nq]
    for i in range(nq):
        lim = int(np.searchsorted(ids, np.uint64(max(int(cur[i]) - 19, 0)), side="left")) if broke[i] else n
        lim = min(lim, n)
        col = S[:lim, i]
        if lim == 0 or col.max() <= 0:
            assert rec["best_id"][i] == 0 and rec["max_score"][i] == 0
            continue
        assert abs(float(rec["max_score"][i]) - col.max()) < SCORE_ATOL
        assert abs(col[int(rec["best_id"][i] - ids[0])] - col.max()) < 2 * SCORE_ATOL


def pkg_breaks(ids, cur):
    from conftest import load_package
    return load_package().sharded_db.shard_breaks(ids, cur)


def test_loop_database_50k_rows(api, oracle, synth):
    """configs[4]'s whole database on ONE GPU: 50 000 key-frames (212.8 MB of descriptors), 512 queries per call."""
    import torch
    n, nq = 50000, 512
    db = synth.lcd_database(n, seed=0x50); ids = np.arange(n, dtype=np.uint64) * 3 + 7
    D = api.LoopDatabase(n)
    t = torch.from_numpy(db).cuda(); D.append_batch(ids, t.data_ptr(), n)
    rng = np.random.default_rng(45)
    q = db[rng.integers(0, n, nq)] * 0.9 + 0.1 * synth.lcd_database(nq, seed=80)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    cur = np.full(nq, int(ids[-1]) + 20, np.uint64)
    cur[::7] = rng.integers(100, int(ids[-1]) + 40, len(cur[::7])).astype(np.uint64)
    dq = torch.from_numpy(q).cuda()
    dbest = torch.zeros(nq, dtype=torch.int64, device="cuda"); dmax = torch.zeros(nq, device="cuda"); dcnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    D.query_batch(dq.data_ptr(), cur, nq, dbest.data_ptr(), dmax.data_ptr(), dcnt.data_ptr())
    torch.cuda.synchronize()
    _db_check(oracle, db, ids, q, cur, dbest.cpu().numpy(), dmax.cpu().numpy(), dcnt.cpu().numpy(), list(range(0, nq, 16)))
    one = D.query(q[3], int(cur[3]))                                     # the B = 1 entry point on the same database
    assert one[0] == int(dbest[3]) and abs(one[1] - float(dmax[3])) < SCORE_ATOL


def test_sharded_records_merge_on_device_equals_one_scan(api, oracle, synth):
    """8 id-range shards on one GPU: per-shard records from myslam_lcddb_query_batch_sharded, reduced by
    myslam_lcd_merge_candidates_device, equal ONE scan of the whole database — including queries whose scan breaks inside shard 3
    (everything behind it must be ignored) and a duplicate row in a later shard (the lowest id wins)."""
    import torch
    S, per, nq = 8, 300, 96
    n = S * per
    db = synth.lcd_database(n, seed=0x51); ids = np.arange(n, dtype=np.uint64) * 2
    db[5 * per + 11] = db[17]
    rng = np.random.default_rng(46)
    q = db[rng.integers(0, n, nq)] * 0.9 + 0.1 * synth.lcd_database(nq, seed=81)
    q[0] = db[17]; q[1] = db[5 * per + 7]
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    cur = rng.integers(30, 2 * n + 40, nq).astype(np.uint64)
    cur[0] = 2 * n + 20
    cur[1] = ids[3 * per + per // 2] + 9                                 # best match in shard 5, break inside shard 3
    cur[2] = ids[3 * per] + 19                                           # break at the first row of shard 3
    dq = torch.from_numpy(q).cuda()
    gathered = torch.zeros(S * nq * 16, dtype=torch.uint8, device="cuda")
    shards = []
    for s in range(S):
        D = api.LoopDatabase(per)
        t = torch.from_numpy(db[s * per:(s + 1) * per].copy()).cuda(); D.append_batch(ids[s * per:(s + 1) * per], t.data_ptr(), per)
        D.query_batch_sharded(dq.data_ptr(), cur, nq, gathered.data_ptr() + s * nq * 16)
        shards.append((D, t))
    dbest = torch.zeros(nq, dtype=torch.int64, device="cuda"); dmax = torch.zeros(nq, device="cuda"); dcnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    api.lcd_merge_candidates_device(gathered.data_ptr(), S, nq, dbest.data_ptr(), dmax.data_ptr(), dcnt.data_ptr())
    torch.cuda.synchronize()
    hb, hm, hc = api.lcd_merge_candidates(gathered.cpu().numpy().view(api.CAND_DTYPE).reshape(S, nq))      # the host entry point agrees
    assert np.array_equal(hb.view(np.int64), dbest.cpu().numpy()) and np.array_equal(hm, dmax.cpu().numpy()) and np.array_equal(hc, dcnt.cpu().numpy())
    _db_check(oracle, db, ids, q, cur, dbest.cpu().numpy(), dmax.cpu().numpy(), dcnt.cpu().numpy(), range(nq))
    assert int(dbest[0]) == 34 and int(dbest[1]) < int(ids[3 * per + per // 2])


@pytest.mark.parametrize("h,w", [(376, 1241), (120, 160), (97, 131), (480, 640), (33, 41), (200, 9), (9, 300)])
def test_fused_input_equals_two_pass_blur(api, synth, h, w):
    """blur_in_place = False evaluates only the blurred pixels the 160 x 120 resize reads (k_lcd_input_fused); blur_in_place = True
    runs the full Gaussian and the resize.  Both are exact integer arithmetic: identical network input, identical descriptor bits."""
    lcd = api.DeepLCD(synth.calc_weights())
    img = synth.random_image(h * 1000 + w, h, w)
    d1, _ = lcd.calcDescrOriginalImg(img, blur_in_place=False)
    d2, _ = lcd.calcDescrOriginalImg(img.copy(), blur_in_place=True)
    assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32))


def test_fused_kernels_against_the_generic_layer_kernels(api, oracle, synth):
    """The fused kernels (conv1 + pool + LRN, split-precision matrix-core conv2, pool + LRN, conv3 + norm) and the generic layer-by-layer kernels run the
    same layer list: descriptors agree to float noise, and both sit within the tolerance of the oracle."""
    w = synth.calc_weights()
    fused, generic = api.DeepLCD(w), api.DeepLCD(w)
    generic.set_option(generic.OPT_GENERIC_KERNELS, 1)
    assert fused.uses_fused_kernels() and not generic.uses_fused_kernels()
    for i in range(3):
        img = synth.random_image(4100 + i, 240, 320)
        a, _ = fused.calcDescrOriginalImg(img); b, _ = generic.calcDescrOriginalImg(img)
        ref = oracle.calc_forward(w, oracle.calc_preproc(img, blur_in_place=True)[0])
        assert np.abs(a - b).max() < 5e-6 and np.abs(a - ref).max() < DESC_ATOL and np.abs(b - ref).max() < DESC_ATOL
    x = np.random.default_rng(3).random((120, 160), dtype=np.float32)
    for stage in range(5):                                          # the stage taps agree between the two kernel families
        ta, tb = fused.debug_forward(x, stage), generic.debug_forward(x, stage)
        assert np.abs(ta - tb).max() <= 2e-5 * max(1.0, float(np.abs(tb).max())), stage


def test_create_from_caffe_files(api, oracle, synth, tmp_path):
    """DeepLCD(prototxt, caffemodel) as the reference constructs it (deeplcd.cpp:10-31): a hand-encoded deploy.prototxt + .caffemodel
    pair (tests/caffe_files.py, no Caffe) gives the flat-blob handle's descriptor bit for bit."""
    import caffe_files
    w = synth.calc_weights()
    pp, mp = caffe_files.write_pair(tmp_path, api.calc_default_layers(), w)
    a, b = api.DeepLCD.from_caffe(pp, mp), api.DeepLCD(w)
    assert a.uses_fused_kernels()
    img = synth.random_image(77, 376, 1241)
    da, _ = a.calcDescrOriginalImg(img); db, _ = b.calcDescrOriginalImg(img)
    assert np.array_equal(da.view(np.uint32), db.view(np.uint32))
    # the CALCW2 model file (records + weights) loads to the same handle
    L = api.calc_default_layers()
    path = str(tmp_path / "calc.w2")
    with open(path, "wb") as f:
        f.write(b"CALCW2\0\0"); f.write(np.uint32(len(L)).tobytes()); f.write(L.tobytes())
        f.write(np.uint64(w.size).tobytes()); f.write(np.asarray(w, np.float32).tobytes())
    dc, _ = api.DeepLCD(path=path).calcDescrOriginalImg(img)
    assert np.array_equal(dc.view(np.uint32), db.view(np.uint32))


@pytest.mark.parametrize("change", ["alpha", "beta_k", "no_relu3", "lrn3", "no_lrn"])
def test_layer_list_is_data(api, oracle, synth, tmp_path, change):
    """A changed hyper-parameter in the prototxt changes the output exactly as the oracle's layer-list forward predicts: LRN alpha
    (fused kernels, fast pow), beta / k (fused kernels, powf), a dropped ReLU (flag), an LRN window of 3 and a net without LRN layers
    (generic layer kernels)."""
    import caffe_files
    w = synth.calc_weights()
    L = api.calc_default_layers()
    if change == "alpha":
        L["alpha"][3] = 0.5; L["alpha"][7] = 2.0
    elif change == "beta_k":
        L["beta"][3] = 0.5; L["k"][3] = 2.0; L["beta"][7] = 1.25; L["alpha"][7] = 1.0
    elif change == "no_relu3":
        L = L[:-1]
    elif change == "lrn3":
        L["local_size"][3] = 3; L["alpha"][3] = 0.3
    else:
        L = L[[0, 1, 2, 4, 5, 6, 8, 9]]
    pp, mp = caffe_files.write_pair(tmp_path, L, w)
    lcd = api.DeepLCD.from_caffe(pp, mp)
    assert lcd.uses_fused_kernels() == (change != "lrn3")
    base = api.DeepLCD(w)
    for i in range(2):
        img = synth.random_image(500 + i, 200, 300)
        x, _ = oracle.calc_preproc(img, blur_in_place=True)
        got, _ = lcd.calcDescrOriginalImg(img)
        ref = oracle.calc_forward_net(L, w, x)
        assert np.abs(got - ref).max() < DESC_ATOL, change
        if change != "no_relu3" or (oracle.calc_forward(w, x) != ref).any():
            assert np.abs(got - base.calcDescrOriginalImg(img)[0]).max() > 10 * DESC_ATOL or change == "no_lrn", change


def test_unsupported_models_are_refused(api, synth):
    w = synth.calc_weights()
    L = api.calc_default_layers()
    bad = L.copy(); bad["type"][2] = 9
    with pytest.raises(api.MyslamError) as e:
        api.DeepLCD(w, layers=bad)
    assert e.value.code == api.ERR_UNSUPPORTED
    bad = L.copy(); bad["pad"][8] = 1                               # 4 x 16 x 21 outputs instead of 1064
    with pytest.raises(api.MyslamError) as e:
        api.DeepLCD(w, layers=bad)
    assert e.value.code == api.ERR_UNSUPPORTED
    with pytest.raises(api.MyslamError) as e:                       # weights that do not fit the list
        api.DeepLCD(w[:-1], layers=L)
    assert e.value.code == api.ERR_INVALID


def test_conv2_f16x3_and_bf16x6_agree_and_ranges_select_the_kernel(api, oracle, synth):
    """conv2 of the fused path has two matrix-core forms with f32-level accuracy: three products of f16 pieces (the default when the model's
    ranges fit f16) and six of bf16 pieces.  Same model: both within the oracle's tolerance and within float noise of each other.  A model whose
    conv2 weights reach 40 cannot put 2^11 h into f16: it must take the bf16 kernel by itself and still match the oracle."""
    w = synth.calc_weights()
    a, b = api.DeepLCD(w), api.DeepLCD(w)
    b.set_option(b.OPT_CONV2_BF16X6, 1)
    assert a.conv2_products() == 3 and b.conv2_products() == 6
    x = np.random.default_rng(11).random((120, 160), dtype=np.float32)
    ta, tb = a.debug_forward(x, 2), b.debug_forward(x, 2)                     # conv2 + ReLU output
    assert np.abs(ta - tb).max() <= 4e-6 * float(np.abs(tb).max())
    for i in range(2):
        img = synth.random_image(5200 + i, 240, 320)
        da, _ = a.calcDescrOriginalImg(img); db_, _ = b.calcDescrOriginalImg(img)
        ref = oracle.calc_forward(w, oracle.calc_preproc(img, blur_in_place=True)[0])
        assert np.abs(da - db_).max() < 5e-6 and np.abs(da - ref).max() < DESC_ATOL and np.abs(db_ - ref).max() < DESC_ATOL
    big = w.copy()
    o2 = 64 * 25 + 64                                                          # conv2 weights follow conv1's 64 x 25 weights + 64 biases
    big[o2:o2 + 128 * 64 * 16] *= 40.0 / float(np.abs(big[o2:o2 + 128 * 64 * 16]).max())
    c = api.DeepLCD(big)
    assert c.uses_fused_kernels() and c.conv2_products() == 6
    img = synth.random_image(5300, 240, 320)
    dc, _ = c.calcDescrOriginalImg(img)
    assert np.abs(dc - oracle.calc_forward(big, oracle.calc_preproc(img, blur_in_place=True)[0])).max() < DESC_ATOL
