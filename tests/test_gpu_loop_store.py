"""api.LoopKeyFrameStore (myslam_loop_store_*, myslam_loop_detect_batch) on the device against the numpy restatement of tests/loop_store_ref.py.
Every input array is random in every byte, slots beyond the counts included; every output buffer is pre-filled with 0xA5 bytes and compared WHOLE,
byte for byte, so a write past a count, into a rejected item or into a neighbour shows.  cap 40 takes the 16-byte copy path for every item
(40 * 28 is a multiple of 16), cap 37 the dword path for every item whose base is not 16-byte aligned."""
import numpy as np
import pytest

import loop_store_ref as R

gpu = pytest.mark.gpu
THR = np.float32(0.94)
FIVE_IDS = [3, 4, 10, 11, 2 ** 40 + 1]
KEYS = ("desc", "n_loop", "pyr", "lm", "slot", "status")


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == R.KP_DTYPE:
        a = a.view(np.uint8).reshape(a.shape + (28,))
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def _code(api, fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0
    except api.MyslamError as e:
        return e.code


class Pair:
    """the device store and the restatement, fed the same calls"""

    def __init__(self, api, kf_capacity, cap, feat_cap, stream=None):
        self.api, self.cap, self.feat_cap = api, cap, feat_cap
        self.dev = api.LoopKeyFrameStore(kf_capacity, cap, feat_cap, stream)
        self.ref = R.Store(kf_capacity, cap, feat_cap)
        self.keep = []                       # device inputs of calls that may still be in flight

    def put(self, ids, kps, desc, counts, status, lm, n_feat):
        t = [_dev(kps), _dev(desc), _dev(np.asarray(counts, np.int32)), None if status is None else _dev(np.asarray(status, np.int32)), _dev(lm),
             _dev(np.asarray(n_feat, np.int32))]
        self.keep.append(t)
        code = _code(self.api, self.dev.put_batch, ids, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0 if t[3] is None else t[3].data_ptr(),
                     t[4].data_ptr(), t[5].data_ptr())
        want = self.ref.put(ids, kps, desc, counts, status, lm, n_feat)
        assert code == want and len(self.dev) == len(self.ref), (code, want)
        return code

    def set_landmarks(self, ids, lm, n_feat):
        t = [_dev(lm), _dev(np.asarray(n_feat, np.int32))]
        self.keep.append(t)
        code = _code(self.api, self.dev.set_landmarks_batch, ids, t[0].data_ptr(), t[1].data_ptr())
        assert code == self.ref.set_landmarks(ids, lm, n_feat)
        return code

    def outputs(self, nq):
        return {k: _dev(v) for k, v in R.sentinel_outputs(nq, self.cap, self.feat_cap).items()}

    def launch(self, q, out, thr_high=THR, max_suspected=3):
        self.dev.detect_batch(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), len(q[0]), out["desc"].data_ptr(), out["n_loop"].data_ptr(),
                              out["pyr"].data_ptr(), out["lm"].data_ptr(), out["slot"].data_ptr(), out["status"].data_ptr(), thr_high, max_suspected)

    def detect(self, best, score, cnt, thr_high=THR, max_suspected=3):
        """one call on sentinel-filled outputs -> {name: bytes}; asserts that the restatement gives the same bytes"""
        import torch
        best, score, cnt = np.asarray(best, np.uint64), np.asarray(score, np.float32), np.asarray(cnt, np.int32)
        q = [_dev(best), _dev(score), _dev(cnt)]
        out = self.outputs(len(best))
        self.launch(q, out, thr_high, max_suspected)
        torch.cuda.synchronize()
        got = {k: out[k].cpu().numpy().tobytes() for k in KEYS}
        want = self.ref.detect(best, score, cnt, thr_high, max_suspected, R.sentinel_outputs(len(best), self.cap, self.feat_cap))
        for k in KEYS:
            assert got[k] == want[k].tobytes(), k
        return got, want


def five(api, cap, feat_cap=16, kf_capacity=8):
    """five key-frames in two puts: counts 0, 1, cap - 1, cap, cap + 3 (stored as cap); n_feat 0, 1, 16, 20 (as 16), -2 (as 0)"""
    p = Pair(api, kf_capacity, cap, feat_cap)
    kps, desc, lm = R.random_keyframes(cap, 5, cap, feat_cap)
    counts, nf = [0, 1, cap - 1, cap, cap + 3], [0, 1, feat_cap, feat_cap + 4, -2]
    assert p.put(FIVE_IDS[:2], kps[:2], desc[:2], counts[:2], None, lm[:2], nf[:2]) == 0
    assert p.put(FIVE_IDS[2:], kps[2:], desc[2:], counts[2:], [0, 0, 0], lm[2:], nf[2:]) == 0
    assert len(p.dev) == 5 and p.dev.capacity() == kf_capacity
    return p


def full_query():
    """nine queries: every stored id, one of them twice, one id that is not stored, one rejected by its score, one by its count"""
    best = FIVE_IDS + [FIVE_IDS[3], 5, FIVE_IDS[2], FIVE_IDS[3]]
    score = [0.95, 0.99, 1.0, 0.97, 0.96, 0.97, 0.99, 0.5, 0.99]
    cnt = [0, 1, 2, 3, 0, 1, 0, 0, 4]
    return best, score, cnt


@gpu
@pytest.mark.parametrize("cap", [40, 37])
def test_gather_both_copy_paths(api, cap):
    p = five(api, cap)
    got, want = p.detect(*full_query())
    assert want["status"].tolist() == [0] * 6 + [-1, 1, 1] and want["n_loop"].tolist() == [0, 1, cap - 1, cap, cap, cap, 0, 0, 0]
    assert want["slot"].tolist() == [0, 1, 2, 3, 4, 3, -1, -1, -1]
    assert (cap * 28) % 16 == (0 if cap == 40 else 12)              # cap 37: items 1, 2, 3 of the caller's key-point table start off a 16-byte boundary
    for k in (3, 2, 0):                                             # nq = 1: a full key-frame, an odd row count, an empty one
        _, w = p.detect([FIVE_IDS[k]], [0.99], [0])
        assert w["status"].tolist() == [0] and w["slot"].tolist() == [k]


@gpu
@pytest.mark.parametrize("cap", [40, 37])
def test_decision_edges(api, cap):
    p = five(api, cap)
    below, above = np.nextafter(THR, np.float32(0)), np.nextafter(THR, np.float32(1))
    score = [THR, below, above, THR, THR, np.nan, np.nan, np.inf, 0.0]
    cnt = [3, 3, 3, 4, -5, 0, 4, 3, 0]
    best = [FIVE_IDS[3]] * 9
    _, w = p.detect(best, score, cnt)
    assert w["status"].tolist() == [0, 1, 0, 1, 0, 0, 1, 0, 1]
    _, w = p.detect(best, score, cnt, max_suspected=2)
    assert w["status"].tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1]
    _, w = p.detect(best, score, cnt, thr_high=np.float32(np.inf))     # a recorded step switched off: only NaN and +inf are not below +inf
    assert w["status"].tolist() == [1, 1, 1, 1, 1, 0, 1, 0, 1]
    _, w = p.detect(best, [1.0] * 9, [0] * 9, thr_high=np.float32(np.inf))
    assert w["status"].tolist() == [1] * 9


@gpu
def test_refused_key_frame_is_stored_with_no_rows(api):
    cap, F = 40, 16
    p = Pair(api, 4, cap, F)
    kps, desc, lm = R.random_keyframes(7, 3, cap, F)
    assert p.put([1, 2, 3], kps, desc, [cap, cap, 5], [0, -3, 7], lm, [F, 4, 2]) == 0
    _, w = p.detect([1, 2, 3], [0.99] * 3, [0] * 3)
    assert w["status"].tolist() == [0, 0, 0] and w["n_loop"].tolist() == [cap, 0, 0] and w["slot"].tolist() == [0, 1, 2]
    assert w["lm"][1, :4].tolist() == lm[1, :4].tolist()            # the landmark table is kept all the same


@gpu
def test_put_errors_leave_the_store_as_it_was(api):
    cap = 37
    p = five(api, cap)
    before, _ = p.detect(*full_query())
    kps, desc, lm = R.random_keyframes(8, 4, cap, 16)
    for ids in ([2 ** 40 + 5, 2 ** 40 + 4], [2 ** 40 + 5, 2 ** 40 + 5], [2 ** 40 + 1], [7, 2 ** 41]):              # descending, repeated, held already, below the last
        assert p.put(ids, kps[:len(ids)], desc[:len(ids)], [cap] * len(ids), None, lm[:len(ids)], [16] * len(ids)) == api.ERR_INVALID
        after, _ = p.detect(*full_query())
        assert after == before and len(p.dev) == 5
    ids = [2 ** 41, 2 ** 41 + 1, 2 ** 41 + 2, 2 ** 41 + 3]                                                          # 5 + 4 > 8: one too many
    assert p.put(ids, kps, desc, [cap] * 4, None, lm, [16] * 4) == api.ERR_CAPACITY
    after, _ = p.detect(*full_query())
    assert after == before and len(p.dev) == 5
    assert p.put(ids[:3], kps[:3], desc[:3], [cap, 2, 0], None, lm[:3], [16, 3, 0]) == 0 and len(p.dev) == 8           # exactly full
    best, score, cnt = full_query()
    _, w = p.detect(best + ids, score + [0.99] * 4, cnt + [0] * 4)
    assert w["status"].tolist()[9:] == [0, 0, 0, -1] and w["slot"].tolist()[9:] == [5, 6, 7, -1]
    assert p.put([2 ** 42], kps[:1], desc[:1], [1], None, lm[:1], [1]) == api.ERR_CAPACITY


@gpu
def test_set_landmarks(api):
    cap, F = 37, 16
    p = five(api, cap)
    _, lm0 = p.detect(*full_query())
    lm = np.random.default_rng(3).integers(-1, 50, (3, F)).astype(np.int32)
    assert p.set_landmarks([FIVE_IDS[4], FIVE_IDS[0], FIVE_IDS[2]], lm, [F + 9, -1, 5]) == 0
    _, w = p.detect(*full_query())
    assert w["lm"][4].tolist() == lm[0].tolist() and w["lm"][2, :5].tolist() == lm[2, :5].tolist()
    assert w["lm"][2, 5:].tobytes() == R.sentinel_outputs(1, cap, F)["lm"][0, 5:].tobytes() and w["lm"][3].tobytes() == lm0["lm"][3].tobytes()
    assert w["pyr"].tobytes() == lm0["pyr"].tobytes() and w["desc"].tobytes() == lm0["desc"].tobytes()              # rows are not touched
    before, _ = p.detect(*full_query())
    for ids in ([FIVE_IDS[1], 5], [FIVE_IDS[1], FIVE_IDS[1]]):                                                        # an id that is not held, an id named twice
        assert p.set_landmarks(ids, lm[:2], [F, F]) == api.ERR_INVALID
        after, _ = p.detect(*full_query())
        assert after == before


@gpu
def test_call_level_errors(api):
    import torch
    cap, F = 40, 16
    INV, CAPY = api.ERR_INVALID, api.ERR_CAPACITY
    for args, code in (((0, cap, F), INV), ((-2, cap, F), INV), ((4, 0, F), INV), ((4, cap, 0), INV), ((4, cap, -1), INV), ((4, 16385, F), CAPY),
                       ((4, cap, 65537), CAPY)):
        with pytest.raises(api.MyslamError) as err:
            api.LoopKeyFrameStore(*args)
        assert err.value.code == code, args
    p = five(api, cap)
    before, _ = p.detect(*full_query())
    kps, desc, lm = R.random_keyframes(9, 1, cap, F)
    t = [_dev(kps), _dev(desc), _dev(np.array([3], np.int32)), _dev(lm), _dev(np.array([2], np.int32))]
    ptr = [x.data_ptr() for x in t]
    put = lambda ids, a: _code(api, p.dev.put_batch, ids, a[0], a[1], a[2], 0, a[3], a[4])
    for k in range(5):                                               # every pointer but d_kf_status
        assert put([2 ** 50], ptr[:k] + [0] + ptr[k + 1:]) == INV, k
    assert put([], ptr) == INV                                       # batch 0
    lib = api.lib()
    ids1 = np.array([2 ** 50], np.uint64)
    assert lib.myslam_loop_store_put_batch(p.dev._h, None, 1, ptr[0], ptr[1], ptr[2], None, ptr[3], ptr[4]) == INV
    assert lib.myslam_loop_store_put_batch(p.dev._h, ids1.ctypes.data, -1, ptr[0], ptr[1], ptr[2], None, ptr[3], ptr[4]) == INV
    assert lib.myslam_loop_store_put_batch(None, ids1.ctypes.data, 1, ptr[0], ptr[1], ptr[2], None, ptr[3], ptr[4]) == INV
    sl = lambda ids, a, b: _code(api, p.dev.set_landmarks_batch, ids, a, b)
    assert sl([FIVE_IDS[0]], 0, ptr[4]) == INV and sl([FIVE_IDS[0]], ptr[3], 0) == INV and sl([], ptr[3], ptr[4]) == INV
    assert lib.myslam_loop_store_set_landmarks_batch(p.dev._h, None, 1, ptr[3], ptr[4]) == INV
    assert lib.myslam_loop_store_set_landmarks_batch(p.dev._h, ids1.ctypes.data, -1, ptr[3], ptr[4]) == INV
    assert len(p.dev) == 5
    # detect: every pointer, nq <= 0, nq beyond the launch grid
    best, score, cnt = full_query()
    q = [_dev(np.asarray(best, np.uint64)), _dev(np.asarray(score, np.float32)), _dev(np.asarray(cnt, np.int32))]
    out = p.outputs(9)
    a = [q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), 9, out["desc"].data_ptr(), out["n_loop"].data_ptr(), out["pyr"].data_ptr(),
         out["lm"].data_ptr(), out["slot"].data_ptr(), out["status"].data_ptr()]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        assert _code(api, p.dev.detect_batch, *(a[:k] + [0] + a[k + 1:])) == INV, k
    for nq, code in ((0, INV), (-1, INV), (65536, CAPY)):
        assert _code(api, p.dev.detect_batch, *(a[:3] + [nq] + a[4:])) == code, nq
    assert lib.myslam_loop_detect_batch(None, a[0], a[1], a[2], 9, 0.94, 3, *a[4:]) == INV
    torch.cuda.synchronize()
    fresh = R.sentinel_outputs(9, cap, F)
    assert all(out[k].cpu().numpy().tobytes() == fresh[k].tobytes() for k in KEYS)                                    # nothing was enqueued
    after, _ = p.detect(*full_query())
    assert after == before


@gpu
def test_limit_shape(api):
    """cap 16384 and feat_cap 65536, the matcher's limits: one full key-frame in a store of two, one query; a second query for the empty slot's id"""
    cap, F = 16384, 65536
    p = Pair(api, 2, cap, F)
    kps, desc, lm = R.random_keyframes(11, 1, cap, F)
    assert p.put([2 ** 63], kps, desc, [cap], [0], lm, [F]) == 0
    _, w = p.detect([2 ** 63], [0.99], [1])
    assert w["status"].tolist() == [0] and w["n_loop"].tolist() == [cap] and w["pyr"].tobytes() == kps.tobytes() and w["lm"].tobytes() == lm.tobytes()
    _, w = p.detect([2 ** 63 + 1], [0.99], [1])
    assert w["status"].tolist() == [-1]


@gpu
def test_recorded(api):
    """detect_batch recorded into a StepGraph replays the eager bytes; ids, counts and the number of key-frames held are read on the device, so after
    a later put_batch a replay with d_best_id rewritten returns the new key-frame; put_batch and set_landmarks_batch on the capturing stream are refused and the recording goes on"""
    import torch
    cap, F = 37, 16
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p = Pair(api, 8, cap, F, stream=stream.cuda_stream)
        kps, desc, lm = R.random_keyframes(cap, 5, cap, F)
        assert p.put(FIVE_IDS, kps, desc, [0, 1, cap - 1, cap, cap + 3], None, lm, [0, 1, F, F + 4, -2]) == 0
        best, score, cnt = full_query()
        eager, _ = p.detect(best, score, cnt)
        q = [_dev(np.asarray(best, np.uint64)), _dev(np.asarray(score, np.float32)), _dev(np.asarray(cnt, np.int32))]
        out = p.outputs(9)
        new = R.random_keyframes(12, 1, cap, F)
        tnew = [_dev(new[0]), _dev(new[1]), _dev(np.array([cap - 2], np.int32)), _dev(new[2]), _dev(np.array([7], np.int32))]
        refused = []

        def body():
            refused.append(_code(api, p.dev.put_batch, [2 ** 45], tnew[0].data_ptr(), tnew[1].data_ptr(), tnew[2].data_ptr(), 0, tnew[3].data_ptr(),
                                 tnew[4].data_ptr()))
            refused.append(_code(api, p.dev.set_landmarks_batch, [FIVE_IDS[1]], tnew[3].data_ptr(), tnew[4].data_ptr()))
            p.launch(q, out)

        g = api.StepGraph.record(stream.cuda_stream, [], body)
        assert refused == [api.ERR_UNSUPPORTED] * 2 and len(p.dev) == 5 and g.node_count() >= 1
        torch.cuda.synchronize()
        fresh = R.sentinel_outputs(9, cap, F)
        assert all(out[k].cpu().numpy().tobytes() == fresh[k].tobytes() for k in KEYS)          # recording ran nothing
        g.launch(stream.cuda_stream)
        torch.cuda.synchronize()
        assert {k: out[k].cpu().numpy().tobytes() for k in KEYS} == eager
        # a key-frame put after the recording
        new_id = 2 ** 45
        assert p.put([new_id], new[0], new[1], [cap - 2], None, new[2], [7]) == 0
        best2 = list(best); best2[6] = new_id; best2[0] = new_id                                 # the unknown id's item, and one more
        q[0].copy_(_dev(np.asarray(best2, np.uint64)))
        for k, v in p.outputs(9).items():
            out[k].copy_(v)
        g.launch(stream.cuda_stream)
        torch.cuda.synchronize()
        want = p.ref.detect(np.asarray(best2, np.uint64), np.asarray(score, np.float32), cnt, THR, 3, R.sentinel_outputs(9, cap, F))
        assert want["status"].tolist() == [0] * 7 + [1, 1] and want["slot"].tolist()[6] == 5 and want["n_loop"].tolist()[6] == cap - 2
        for k in KEYS:
            assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k


@gpu
def test_many_items_split_over_few_chunks(api):
    """1024 key-frames of cap 1022 put in ONE call and gathered by ONE call of 1024 queries.  With that many items a call launches two workgroups per
    item, so every lane makes more than three accesses per array and the four-way unrolled loop of the copy runs (1788 / 2044 16-byte pieces and
    7154 dwords against 3 x 2 x 256 = 1536), in both kernels, split over two chunks, on the 16-byte path (even items of the caller's key-point
    table: 1022 x 28 b is a multiple of 16 for even b) and on the dword path (odd items)."""
    cap, F, N = 1022, 16, 1024
    assert -(-2048 // N) == 2 and (cap * 28 // 16) > 1536 and (cap * 28) % 16 == 8
    p = Pair(api, N, cap, F)
    kps, desc, lm = R.random_keyframes(21, N, cap, F)
    counts = np.full(N, cap, np.int32); counts[::7] = cap - 1; counts[5] = 0; counts[6] = 800; counts[9] = cap + 1
    nf = np.full(N, F, np.int32); nf[::5] = 3
    ids = (np.arange(N) * 3 + 1).astype(np.uint64)
    assert p.put(ids, kps, desc, counts, None, lm, nf) == 0
    order = np.random.default_rng(22).permutation(N)
    score = np.full(N, 0.99, np.float32); score[::50] = 0.5
    best = ids[order].copy(); best[7] = 2                                # an id that is not held, in the middle of the batch
    _, want = p.detect(best, score, np.zeros(N, np.int32))
    slot = np.where(score < THR, -1, order); slot[7] = -1
    assert want["slot"].tolist() == slot.tolist() and (want["status"] == 0).sum() == N - 22
    assert want["n_loop"][slot >= 0].tolist() == np.minimum(counts, cap)[order][slot >= 0].tolist()


@gpu
def test_descriptor_pointer_off_a_dword_boundary(api):
    """d_loop_desc is a byte pointer: one byte past a 16-byte boundary the descriptors go byte by byte, and no byte on either side changes"""
    import torch
    cap, F = 37, 16
    p = five(api, cap)
    best, score, cnt = full_query()
    q = [_dev(np.asarray(best, np.uint64)), _dev(np.asarray(score, np.float32)), _dev(np.asarray(cnt, np.int32))]
    out = p.outputs(9)
    nbytes = 9 * cap * 32
    raw = _dev(np.full(nbytes + 16, 0xA5, np.uint8))
    assert raw.data_ptr() % 16 == 0
    p.dev.detect_batch(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), 9, raw.data_ptr() + 1, out["n_loop"].data_ptr(), out["pyr"].data_ptr(),
                       out["lm"].data_ptr(), out["slot"].data_ptr(), out["status"].data_ptr())
    torch.cuda.synchronize()
    want = p.ref.detect(np.asarray(best, np.uint64), np.asarray(score, np.float32), cnt, THR, 3, R.sentinel_outputs(9, cap, F))
    r = raw.cpu().numpy()
    assert r[1:1 + nbytes].tobytes() == want["desc"].tobytes() and r[0] == 0xA5 and (r[1 + nbytes:] == 0xA5).all()
    for k in KEYS:
        if k != "desc":
            assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k


# ------------------------------------------------------------------------------------------ the chain
CH_CAP, CH_FEAT, CH_OUT, CH_LEVELS = 512, 64, 64, 8           # the shapes of tests/test_gpu_loop_match.py
CH_IDS = [3, 7, 10, 14, 21, 30]
CH_NFEAT = [64, 64, 64, 64, 60, 64]
CH_HITS = [1, None, 3, 4, 1]                                   # the key-frame each query is made to resemble; None: none of them
CH_LAND = 6 * CH_FEAT


def chain_scene(synth):
    """six key-frames and five queries.  Key-frame k sees CH_NFEAT[k] features, eight pyramid rows each; feature f names landmark 64 k + (63 - f) unless
    f % 7 == 6; key-frame 3 keeps a map point for nine features only.  The landmarks of key-frame k and the pixels of a current key-frame that looks
    at them are one synth.pnp_problem.  A query's image descriptor is its key-frame's with 3 % of another vector mixed in."""
    db = synth.lcd_database(6, seed=0x10C)
    noise = synth.lcd_database(len(CH_HITS), seed=0x10D)
    kfs, pos, K = [], np.full((CH_LAND, 3), np.nan), None
    for k, n in enumerate(CH_NFEAT):
        slots = CH_FEAT * k + np.arange(n)[::-1]
        lm = np.where(np.arange(n) < 9, slots, -1) if k == 3 else np.where(np.arange(n) % 7 == 6, -1, slots)
        loop_desc, loop_cls, cur_desc, cur_cls, lm = R.matching_keyframe(500 + k, n, CH_LEVELS, lm)
        pw, uv, K, _, _ = synth.pnp_problem(n, 0.3, 0.5, seed=40 + k)
        pos[lm[lm >= 0]] = pw[lm >= 0].astype(np.float64) + 1e-9
        kps = np.frombuffer(np.random.default_rng(600 + k).integers(0, 256, len(loop_cls) * 28, dtype=np.uint8).tobytes(), R.KP_DTYPE).copy()
        kps["class_id"] = loop_cls
        kfs.append(dict(kps=kps, desc=loop_desc, lm=lm, cur_desc=cur_desc, cur_cls=cur_cls, uv=uv.astype(np.float32)))
    q = np.stack([noise[b] if k is None else 0.97 * db[k] + 0.03 * noise[b] for b, k in enumerate(CH_HITS)])
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return db, kfs, pos, K, q


def chain_store_inputs(kfs):
    B = len(kfs)
    kps, desc, lm = R.random_keyframes(99, B, CH_CAP, CH_FEAT)
    for k, kf in enumerate(kfs):
        n = len(kf["kps"])
        kps[k, :n] = kf["kps"]; desc[k, :n] = kf["desc"]; lm[k, :len(kf["lm"])] = kf["lm"]
    return kps, desc, [len(kf["kps"]) for kf in kfs], lm, [len(kf["lm"]) for kf in kfs]


def test_chain_inputs_produce_the_mix(synth):
    """CPU: with scores far from both thresholds the scan names the intended key-frames, the restatement's decision gives four candidates and one
    NO_LOOP, and the candidate from key-frame 3 has 64 matched features but nine map points"""
    db, kfs, pos, K, q = chain_scene(synth)
    s = q.astype(np.float64) @ db.astype(np.float64).T
    for b, k in enumerate(CH_HITS):
        if k is None:
            assert s[b].max() < 0.85
        else:
            assert s[b, k] > 0.97 and np.delete(s[b], k).max() < 0.85
    st = R.Store(8, CH_CAP, CH_FEAT)
    assert st.put(CH_IDS, *chain_store_inputs(kfs)[:3], None, *chain_store_inputs(kfs)[3:]) == 0
    best = np.array([CH_IDS[int(np.argmax(r))] for r in s], np.uint64)
    out = st.detect(best, s.max(1).astype(np.float32), (s > 0.92).sum(1).astype(np.int32), THR, 3, R.sentinel_outputs(5, CH_CAP, CH_FEAT))
    assert out["status"].tolist() == [0, 1, 0, 0, 0] and out["slot"].tolist() == [1, -1, 3, 4, 1] and out["n_loop"].tolist() == [512, 0, 512, 480, 512]
    assert (out["lm"][2, :64] >= 0).sum() == 9 and (out["lm"][0, :64] >= 0).sum() == 55 and len(set(kfs[3]["kps"]["class_id"].tolist())) == 64


@gpu
def test_chain_scan_detect_match_verify(api, synth):
    """LoopDatabase.query_batch -> detect_batch -> loop_match_batch -> PnPSolver.verify_batch enqueued on one stream with no host read in between,
    against the same matcher and verifier fed with loop-side arrays assembled on the host (numpy indexing) from the downloaded scan results: every
    output of both stages byte for byte"""
    import torch
    db, kfs, pos, K, q = chain_scene(synth)
    B, cap, F, OUT = len(CH_HITS), CH_CAP, CH_FEAT, CH_OUT
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        D = api.LoopDatabase(16, stream=s)
        t_db = _dev(db); D.append_batch(np.asarray(CH_IDS, np.uint64), t_db.data_ptr(), 6)
        p = Pair(api, 8, cap, F, stream=s)
        kps, desc, counts, lm, nf = chain_store_inputs(kfs)
        assert p.put(CH_IDS, kps, desc, counts, None, lm, nf) == 0
        solver = api.PnPSolver(B, OUT, 100, stream=s)
        # the current side of every item
        cd = np.full((B, cap, 32), 0xFF, np.uint8); cp = np.frombuffer(b"\xff" * (B * cap * 28), R.KP_DTYPE).reshape(B, cap).copy()
        nc = np.zeros(B, np.int32); xy = np.full((B, F, 2), np.nan, np.float32)
        for b, k in enumerate(CH_HITS):
            kf = kfs[0 if k is None else k]
            n = len(kf["cur_cls"])
            cd[b, :n] = kf["cur_desc"]; cp[b, :n] = 0; cp["class_id"][b, :n] = kf["cur_cls"]; nc[b] = n; xy[b, :len(kf["uv"])] = kf["uv"]
        t_cd, t_cp, t_nc, t_xy, t_pos, t_q = _dev(cd), _dev(cp), _dev(nc), _dev(xy), _dev(pos), _dev(q)
        cur_ids = np.arange(200, 200 + B, dtype=np.uint64)
        z = lambda *sh, dt=torch.int32: torch.zeros(*sh, dtype=dt, device="cuda")

        def stage_outputs():
            m = dict(ti=z(B, cap), dist=z(B, cap), pairs=z(B, cap, 2), np=z(B), valid=z(B, OUT, 2), p3=z(B, OUT, 3), p2=z(B, OUT, 2), cnt=z(B), st=z(B))
            v = dict(pose=z(B, 7, dt=torch.float64), flag=z(B, OUT, dt=torch.uint8), ninl=z(B), st=z(B))
            for x in list(m.values()) + [v["ninl"], v["st"]]:
                x.fill_(-7)
            v["pose"].fill_(0.25); v["flag"].fill_(255)
            return m, v

        def match_verify(loop, m, v):
            api.loop_match_batch(loop["desc"].data_ptr(), loop["n_loop"].data_ptr(), t_cd.data_ptr(), t_nc.data_ptr(), loop["pyr"].data_ptr(), t_cp.data_ptr(),
                                 B, cap, t_xy.data_ptr(), loop["lm"].data_ptr(), F, t_pos.data_ptr(), 0, CH_LAND, 10, OUT, m["ti"].data_ptr(),
                                 m["dist"].data_ptr(), m["pairs"].data_ptr(), m["np"].data_ptr(), m["valid"].data_ptr(), m["p3"].data_ptr(),
                                 m["p2"].data_ptr(), m["cnt"].data_ptr(), m["st"].data_ptr(), s)
            solver.verify_batch(m["p3"].data_ptr(), m["p2"].data_ptr(), m["cnt"].data_ptr(), B, K, v["pose"].data_ptr(), v["flag"].data_ptr(),
                                v["ninl"].data_ptr(), v["st"].data_ptr())

        # the device chain: four enqueues, nothing read in between
        scan = dict(best=z(B, dt=torch.int64), mx=z(B, dt=torch.float32), cnt=z(B))
        loop = p.outputs(B)
        m1, v1 = stage_outputs()
        D.query_batch(t_q.data_ptr(), cur_ids, B, scan["best"].data_ptr(), scan["mx"].data_ptr(), scan["cnt"].data_ptr())
        p.launch([scan["best"], scan["mx"], scan["cnt"]], loop)
        match_verify(loop, m1, v1)
        torch.cuda.synchronize()
        # the host path: the decision and the gather by numpy indexing on the downloaded scan results
        best, mx, cnt = scan["best"].cpu().numpy().view(np.uint64), scan["mx"].cpu().numpy(), scan["cnt"].cpu().numpy()
        assert best.tolist() == [CH_IDS[1], best[1], CH_IDS[3], CH_IDS[4], CH_IDS[1]] and cnt.tolist() == [1, 0, 1, 1, 1] and mx[1] < 0.85 < 0.97 < mx[0]
        host = R.sentinel_outputs(B, cap, F)
        for b in range(B):
            if mx[b] < THR or cnt[b] > 3:
                host["n_loop"][b], host["slot"][b], host["status"][b] = 0, -1, 1
                continue
            k = CH_IDS.index(int(best[b])); n = counts[k]
            host["n_loop"][b], host["slot"][b], host["status"][b] = n, k, 0
            host["pyr"][b, :n] = kps[k, :n]; host["desc"][b, :n] = desc[k, :n]; host["lm"][b, :nf[k]] = lm[k, :nf[k]]
        for k in KEYS:
            assert loop[k].cpu().numpy().tobytes() == host[k].tobytes(), k
        m2, v2 = stage_outputs()
        match_verify({k: _dev(x) for k, x in host.items()}, m2, v2)
        torch.cuda.synchronize()
        for a, b_ in ((m1, m2), (v1, v2)):
            for k in a:
                assert a[k].cpu().numpy().tobytes() == b_[k].cpu().numpy().tobytes(), k
        assert host["status"].tolist() == [0, 1, 0, 0, 0]
        assert m1["st"].cpu().tolist() == [0, 1, 2, 0, 0]                            # OK, NO_LOOP -> FEW_PAIRS, FEW_POINTS, OK, OK
        assert m1["cnt"].cpu().tolist()[1:3] == [0, 9]
        assert v1["st"].cpu().tolist() == [api.VERIFY_CONFIRMED, api.VERIFY_FEW_MATCHES, api.VERIFY_FEW_MATCHES, api.VERIFY_CONFIRMED, api.VERIFY_CONFIRMED]
