"""myslam_loop_match_batch (api.loop_match_batch): LoopClosing::MatchFeatures and the gather of ComputeCorrectPose for a batch of candidates on
the device, against a reference that shares no code with it: oracle.hamming_match for the matcher, then the restatement below (the limit from
min(dist), sorted(set(...)) over (current class_id, loop class_id), a list comprehension for the landmark filter, np.float32(pos)).  The
restatement's pair stage is pinned on the CPU against api.match_feature_pairs (test_restatement_matches_the_host_function).

Everything is compared exactly: train_idx, dist, pairs, n_pairs, valid_pairs, the bits of pts3d / pts2d, counts, status.  Every input slot beyond
an item's counts is 0xFF bytes or NaN (a feature nobody names has a landmark slot far outside the table), every output buffer is pre-filled with
a sentinel, and slots beyond the written counts must still hold it.

Descriptors: one random 256-bit row per feature (random rows lie about 128 bits apart, never below 90 here); a pyramid row that is to match
feature f at distance d is f's row with d bits flipped, so distances up to 50 are exact by construction — the tests assert them on the oracle's
output.  Shapes: cap 512, feat_cap 64, out_cap 64 unless a case needs another; one item at the cap limit 16384."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

CAP, FEAT, OUT, LAND = 512, 64, 64, 64
ISENT = -7                                  # int32 outputs
FSENT = 0x4B1D4B1D                          # bit pattern of the float outputs
LM_UNUSED = np.int32(-0x7F7F7F80)           # landmark slot of a feature no pair may name
OK, FEW_PAIRS, FEW_POINTS, INVALID, CAPACITY = 0, 1, 2, -1, -3


# ------------------------------------------------------------------------------------------ the restatement
def ref_pairs(ti, dist, loop_cls, cur_cls):
    """loopclosing.cpp:175-194 on the matcher's output: (current id, loop id) of the kept rows, as the std::set iterates"""
    lim = max(2.0 * float(min(dist)), 30.0)
    return sorted(set((int(cur_cls[t]), int(loop_cls[i])) for i, (t, d) in enumerate(zip(ti, dist)) if float(d) <= lim))


def ref_gather(pairs, lm, pos, xy):
    """loopclosing.cpp:218-237: pairs whose loop feature has a map point, vLoopPoints3d (cv::Point3f of an f64 position), vCurrentPoints2d"""
    valid = [(c, l) for c, l in pairs if lm[l] != -1]
    with np.errstate(over="ignore"):
        p3 = np.array([pos[lm[l]] for _, l in valid], np.float64).reshape(-1, 3).astype(np.float32)
    p2 = np.array([xy[c] for c, _ in valid], np.float32).reshape(-1, 2)
    return valid, p3, p2


def test_restatement_matches_the_host_function(pkg):
    """CPU: ref_pairs against api.match_feature_pairs (myslam_match_feature_pairs) on 60 x 40 rows of 12 features with ties, duplicates and drops"""
    api = pkg.api
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    cur_cls = rng.integers(0, 12, 40); cur = np.stack([_flip(base[f], int(rng.integers(0, 6)), rng) for f in cur_cls])
    loop_cls = rng.integers(0, 12, 60); loop = np.stack([_flip(base[int(rng.integers(0, 12))], int(rng.integers(0, 45)), rng) for _ in loop_cls])
    d = np.unpackbits(loop[:, None, :] ^ cur[None, :, :], axis=2).sum(2)
    ti = d.argmin(1).astype(np.int32); dist = d.min(1).astype(np.int32)            # the first minimum, as BFMatcher keeps it
    lk = np.zeros(60, api.KP_DTYPE); ck = np.zeros(40, api.KP_DTYPE)
    lk["class_id"] = loop_cls; ck["class_id"] = cur_cls
    got = api.match_feature_pairs(ti, dist, lk, ck)
    want = ref_pairs(ti, dist, loop_cls, cur_cls)
    assert 0 < len(want) < (dist <= max(2.0 * dist.min(), 30.0)).sum() < 60          # rows were dropped, and duplicates collapsed
    assert [tuple(p) for p in got.tolist()] == want


# ------------------------------------------------------------------------------------------ scenes
def _flip(row, d, rng):
    out = row.copy()
    for p in rng.choice(256, d, replace=False):
        out[p >> 3] ^= 1 << (p & 7)
    return out


class Item:
    """one candidate: pyramid rows of both key-frames, the current features' pixels, the loop features' landmark slots, the landmark table"""

    def __init__(self, loop_desc, loop_cls, cur_desc, cur_cls, xy, lm, pos, n_loop=None, n_cur=None):
        self.loop_desc, self.loop_cls = np.asarray(loop_desc, np.uint8).reshape(-1, 32), np.asarray(loop_cls, np.int32)
        self.cur_desc, self.cur_cls = np.asarray(cur_desc, np.uint8).reshape(-1, 32), np.asarray(cur_cls, np.int32)
        self.xy, self.lm, self.pos = np.asarray(xy, np.float32), np.asarray(lm, np.int32), np.asarray(pos, np.float64)
        self.n_loop = len(self.loop_cls) if n_loop is None else n_loop          # the counts the call is given
        self.n_cur = len(self.cur_cls) if n_cur is None else n_cur
        self._match = None


def scene(seed, rows, nfeat=FEAT, cur_order=None, cur_levels=1, lm=None, pos=None, **kw):
    """rows = [(loop feature, current feature, distance)]: loop pyramid rows in that order; current rows = cur_levels rows per feature in cur_order"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (nfeat, 32), dtype=np.uint8)
    cur_cls = np.repeat(np.arange(nfeat) if cur_order is None else np.asarray(cur_order), cur_levels)
    loop_desc = np.stack([_flip(base[f], d, rng) for _, f, d in rows]) if rows else np.zeros((0, 32), np.uint8)
    xy = rng.uniform(0, 1000, (nfeat, 2)).astype(np.float32)
    lm = np.arange(nfeat, dtype=np.int32) if lm is None else lm
    pos = rng.normal(0, 10, (LAND, 3)) if pos is None else pos
    return Item(loop_desc, [g for g, _, _ in rows], base[cur_cls], cur_cls, xy, lm, pos, **kw)


def dup_item():
    """13 feature pairs x 8 pyramid rows each; the current rows lie in descending feature order and loop feature g matches current feature 11 - g, so
    the kept pairs arrive in descending current id; loop features 6 and 12 both match current feature 5"""
    rows = [(g, 11 - g, lvl) for g in range(12) for lvl in range(8)] + [(12, 5, lvl) for lvl in range(8)]
    return scene(1, rows, cur_order=np.arange(FEAT)[::-1], cur_levels=8)


def threshold_items():
    """min_dist 0 (limit 30: a row at 30 kept, at 31 dropped), 20 (limit 40: 40 / 41), 15 (2 * min = 30: 30 / 31); 12 pairs otherwise"""
    out = []
    for seed, (mn, keep, drop) in enumerate([(0, 30, 31), (20, 40, 41), (15, 30, 31)]):
        d = [mn, keep, drop] + [mn + 3] * 10
        out.append(scene(10 + seed, [(g, g, d[g]) for g in range(13)]))
    return out


def kept_item(k, n_rows=None):
    """k rows at distances 0..30 and 20 rows at 50 (n_rows given: that many rows, all kept); loop features below 8 have a map point, so at most 64 survive"""
    lm = np.where(np.arange(FEAT) < 8, np.arange(FEAT), -1).astype(np.int32)
    rows = [(r % 64, (r // 64 * 9 + r) % 64, r % 31) for r in range(k if n_rows is None else n_rows)]
    if n_rows is None:
        rows += [(r % 64, (r + 1) % 64, 50) for r in range(20)]
    return scene(100 + k, rows, lm=lm)


def landmark_items():
    """20 pairs with every second loop feature without a map point (10 survivors = min_matches: OK); 18 pairs (9 survivors: FEW_POINTS, arrays
    written); 9 pairs (FEW_PAIRS)"""
    lm = np.where(np.arange(FEAT) % 2 == 0, np.arange(FEAT)[::-1], -1).astype(np.int32)
    return [scene(200 + n, [(g, (g * 5) % 23, g % 7) for g in range(n)], lm=lm) for n in (20, 18, 9)]


def mixed_items():
    a, b, c = threshold_items()
    return [dup_item(), a, b, c, kept_item(1), kept_item(65), kept_item(257), kept_item(0, n_rows=CAP)] + landmark_items() + \
           [scene(300, [], n_loop=0)]


# ------------------------------------------------------------------------------------------ expectation
def expect(oracle, it, cap=CAP, feat_cap=FEAT, out_cap=OUT, landmark_cap=LAND, min_matches=10, match=None):
    nl, nc = min(max(it.n_loop, 0), cap), min(max(it.n_cur, 0), cap)
    e = dict(nl=nl, pairs=[], valid=None, count=0)
    if nl == 0:
        e["ti"] = e["dist"] = np.zeros(0, np.int32)
    elif nc == 0:
        e["ti"] = e["dist"] = np.full(nl, -1, np.int32)                           # the matcher's "no train row"
    else:
        if match is None and it._match is None:
            it._match = oracle.hamming_match(it.loop_desc[:nl], it.cur_desc[:nc])
        e["ti"], e["dist"] = match or it._match
    if nl == 0 or nc == 0:
        e["status"] = FEW_PAIRS
        return e
    lim = max(2.0 * float(e["dist"].min()), 30.0)
    kept = [(int(it.cur_cls[t]), int(it.loop_cls[i])) for i, (t, d) in enumerate(zip(e["ti"], e["dist"])) if float(d) <= lim]
    if any(not (0 <= c < feat_cap and 0 <= l < feat_cap) for c, l in kept):
        e["status"] = INVALID
        return e
    e["pairs"] = ref_pairs(e["ti"], e["dist"], it.loop_cls, it.cur_cls)
    if len(e["pairs"]) < min_matches:
        e["status"] = FEW_PAIRS
        return e
    if any(not (-1 <= it.lm[l] < landmark_cap) for _, l in e["pairs"]):
        e["status"] = INVALID
        return e
    valid, p3, p2 = ref_gather(e["pairs"], it.lm, it.pos, it.xy)
    if len(valid) > out_cap:
        e["status"] = CAPACITY
        return e
    e.update(valid=valid, p3=p3, p2=p2, count=len(valid), status=FEW_POINTS if len(valid) < min_matches else OK)
    return e


def check(r, b, e, cap=CAP, out_cap=OUT):
    nl, npairs = e["nl"], len(e["pairs"])
    assert np.array_equal(r["ti"][b, :nl], e["ti"]) and np.array_equal(r["dist"][b, :nl], e["dist"]), b
    assert (r["ti"][b, nl:] == ISENT).all() and (r["dist"][b, nl:] == ISENT).all(), b
    assert r["st"][b] == e["status"] and r["cnt"][b] == e["count"] and r["np"][b] == npairs, (b, r["st"][b], r["cnt"][b], r["np"][b], e["status"])
    assert r["pairs"][b, :npairs].tolist() == [list(p) for p in e["pairs"]], b
    assert (r["pairs"][b, npairs:] == ISENT).all(), b
    n = e["count"]
    if e["valid"] is not None:
        assert r["valid"][b, :n].tolist() == [list(p) for p in e["valid"]], b
        assert np.array_equal(r["p3"][b, :n], e["p3"].view(np.int32)) and np.array_equal(r["p2"][b, :n], e["p2"].view(np.int32)), b
    assert (r["valid"][b, n:] == ISENT).all() and (r["p3"][b, n:] == FSENT).all() and (r["p2"][b, n:] == FSENT).all(), b


class Bufs:
    """device inputs (poisoned beyond the counts) and sentinel-filled outputs of one call shape"""

    def __init__(self, api, B, cap=CAP, feat_cap=FEAT, out_cap=OUT, landmark_cap=LAND, shared_table=False):
        import torch
        self.api, self.t, self.B, self.cap, self.feat_cap, self.out_cap, self.landmark_cap, self.shared = api, torch, B, cap, feat_cap, out_cap, landmark_cap, shared_table
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device="cuda")
        self.ld, self.cd = z(B, cap, 32, dt=torch.uint8), z(B, cap, 32, dt=torch.uint8)
        self.lp, self.cp = z(B, cap, 28, dt=torch.uint8), z(B, cap, 28, dt=torch.uint8)
        self.nl, self.nc = z(B), z(B)
        self.xy, self.lm = z(B, feat_cap, 2, dt=torch.float32), z(B, feat_cap)
        self.pos = z(1 if shared_table else B, landmark_cap, 3, dt=torch.float64)
        self.out = dict(ti=z(B, cap), dist=z(B, cap), pairs=z(B, cap, 2), np=z(B), valid=z(B, out_cap, 2), p3=z(B, out_cap, 3), p2=z(B, out_cap, 2),
                        cnt=z(B), st=z(B))

    def load(self, items):
        api, B, cap, F, L = self.api, self.B, self.cap, self.feat_cap, self.landmark_cap
        assert len(items) == B
        ld = np.full((B, cap, 32), 0xFF, np.uint8); cd = ld.copy()
        lp = np.frombuffer(b"\xff" * (B * cap * 28), api.KP_DTYPE).reshape(B, cap).copy(); cp = lp.copy()
        xy = np.full((B, F, 2), np.nan, np.float32); lm = np.full((B, F), LM_UNUSED, np.int32)
        pos = np.full((1 if self.shared else B, L, 3), np.nan)
        for b, it in enumerate(items):
            nl, nc = min(max(it.n_loop, 0), cap), min(max(it.n_cur, 0), cap)      # rows beyond the counts stay poison even where the item has them
            ld[b, :nl] = it.loop_desc[:nl]; lp[b, :nl] = 0; lp["class_id"][b, :nl] = it.loop_cls[:nl]
            cd[b, :nc] = it.cur_desc[:nc]; cp[b, :nc] = 0; cp["class_id"][b, :nc] = it.cur_cls[:nc]
            xy[b, :len(it.xy)] = it.xy; lm[b, :len(it.lm)] = it.lm
            pos[0 if self.shared else b, :len(it.pos)] = it.pos
        t = self.t
        for dst, src in ((self.ld, ld), (self.cd, cd), (self.lp, lp.view(np.uint8).reshape(B, cap, 28)), (self.cp, cp.view(np.uint8).reshape(B, cap, 28)),
                         (self.xy, xy), (self.lm, lm), (self.pos, pos), (self.nl, np.array([it.n_loop for it in items], np.int32)),
                         (self.nc, np.array([it.n_cur for it in items], np.int32))):
            dst.copy_(t.from_numpy(src))
        self.clear()

    def clear(self):
        for k, v in self.out.items():
            v.fill_(FSENT if k in ("p3", "p2") else ISENT)

    def run(self, min_matches=10, stream=0, cap=None, batch=None, null_table=False):
        o = self.out
        self.api.loop_match_batch(self.ld.data_ptr(), self.nl.data_ptr(), self.cd.data_ptr(), self.nc.data_ptr(), self.lp.data_ptr(), self.cp.data_ptr(),
                                  batch or self.B, cap or self.cap, self.xy.data_ptr(), self.lm.data_ptr(), self.feat_cap, 0 if null_table else self.pos.data_ptr(),
                                  0 if self.shared else self.landmark_cap, self.landmark_cap, min_matches, self.out_cap, o["ti"].data_ptr(),
                                  o["dist"].data_ptr(), o["pairs"].data_ptr(), o["np"].data_ptr(), o["valid"].data_ptr(), o["p3"].data_ptr(),
                                  o["p2"].data_ptr(), o["cnt"].data_ptr(), o["st"].data_ptr(), stream)

    def results(self):
        self.t.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}


def run_and_check(api, oracle, items, **shape):
    bufs = Bufs(api, len(items), **shape)
    bufs.load(items); bufs.run()
    r = bufs.results()
    es = [expect(oracle, it, **{k: v for k, v in shape.items() if k != "shared_table"}) for it in items]
    for b, e in enumerate(es):
        check(r, b, e, shape.get("cap", CAP), shape.get("out_cap", OUT))
    return r, es


# ------------------------------------------------------------------------------------------ cases
@gpu
def test_duplicates_and_set_order(api, oracle):
    r, (e,) = run_and_check(api, oracle, [dup_item()])
    assert (e["dist"] <= 7).all() and e["status"] == OK and e["count"] == 13       # 104 kept rows -> 13 pairs
    arrival = [int(dup_item().cur_cls[t]) for t in e["ti"]]
    assert arrival[:96] == sorted(arrival[:96], reverse=True) and arrival[96:] == [5] * 8                     # the kept pairs arrive in descending current id ...
    assert e["pairs"] == [(c, 11 - c) for c in range(5)] + [(5, 6), (5, 12)] + [(c, 11 - c) for c in range(6, 12)]      # ... and leave ascending, ties by loop id


@gpu
def test_threshold_branches(api, oracle):
    r, es = run_and_check(api, oracle, threshold_items())
    for e, (mn, keep, drop) in zip(es, [(0, 30, 31), (20, 40, 41), (15, 30, 31)]):
        assert e["dist"].tolist() == [mn, keep, drop] + [mn + 3] * 10
        assert (1, 1) in e["pairs"] and (2, 2) not in e["pairs"] and len(e["pairs"]) == 12 and e["status"] == OK


@gpu
def test_kept_row_counts_around_the_sort_padding(api, oracle):
    ks = (1, 2, 63, 64, 65, 255, 256, 257)
    r, es = run_and_check(api, oracle, [kept_item(k) for k in ks] + [kept_item(0, n_rows=CAP)])
    for k, e in zip(ks, es):
        assert (e["dist"] <= 30).sum() == k and (e["dist"] == 50).sum() == 20      # k = 1: nothing is kept beyond the minimum row itself
    assert [len(e["pairs"]) for e in es] == [1, 2, 63, 64, 65, 255, 256, 257, 512]
    assert [e["status"] for e in es] == [FEW_PAIRS, FEW_PAIRS, FEW_POINTS] + [FEW_POINTS] * 2 + [OK] * 4
    assert es[-1]["nl"] == CAP and es[-1]["count"] == 64 == OUT


@gpu
def test_kept_row_counts_around_the_1024_thread_block(api, oracle):
    """cap 2048 launches the pair stage with 1024 threads (the counts above cross its 256-thread form's chunk edge): 1023, 1024 and 1025 kept rows,
    as many distinct pairs, and the eighth of them whose loop feature has a map point in the gather"""
    ks = (1023, 1024, 1025)
    r, es = run_and_check(api, oracle, [kept_item(k) for k in ks], cap=2048, out_cap=256)
    for k, e in zip(ks, es):
        assert (e["dist"] <= 30).sum() == k and (e["dist"] == 50).sum() == 20
        assert len(e["pairs"]) == k and e["status"] == OK and e["count"] == k // 64 * 8 + min(k % 64, 8)


@gpu
def test_empty_sides_and_clamped_counts(api, oracle):
    full_loop = kept_item(0, n_rows=CAP); full_loop.n_loop = CAP + 5
    full_cur = scene(7, [(g, g, g % 5) for g in range(20)], cur_levels=8); full_cur.n_cur = CAP + 5
    assert len(full_cur.cur_cls) == CAP
    items = [scene(1, [], n_loop=0), scene(2, [(g, g, 0) for g in range(12)], n_cur=0), scene(3, [(g, g, 0) for g in range(12)], n_loop=-3),
             scene(4, [(g, g, 0) for g in range(12)], n_cur=-3), full_loop, full_cur]
    r, es = run_and_check(api, oracle, items)
    assert [e["status"] for e in es] == [FEW_PAIRS] * 4 + [OK, OK] and [e["count"] for e in es] == [0] * 4 + [64, 20]
    assert [e["nl"] for e in es] == [0, 12, 0, 12, CAP, 20] and (r["ti"][1, :12] == -1).all() and (r["ti"][3, :12] == -1).all()


@gpu
def test_landmark_filter(api, oracle):
    r, es = run_and_check(api, oracle, landmark_items())
    assert [(len(e["pairs"]), e["count"], e["status"]) for e in es] == [(20, 10, OK), (18, 9, FEW_POINTS), (9, 0, FEW_PAIRS)]
    assert es[0]["valid"] == [p for p in es[0]["pairs"] if p[1] % 2 == 0] and es[0]["valid"] != sorted(es[0]["valid"], key=lambda p: p[1])
    assert es[1]["valid"] is not None and es[2]["valid"] is None


@gpu
def test_out_cap_edge(api, oracle):
    """64 pairs with a map point fill out_cap; a 65th (loop feature 0 also matches current feature 1) is MYSLAM_ERR_CAPACITY: nothing truncated"""
    rows = [(g, g, g % 4) for g in range(64)]
    r, es = run_and_check(api, oracle, [scene(40, rows), scene(41, rows + [(0, 1, 2)]), scene(42, rows)])
    assert [(len(e["pairs"]), e["count"], e["status"]) for e in es] == [(64, 64, OK), (65, 0, CAPACITY), (64, 64, OK)]


@gpu
def test_bad_indices(api, oracle):
    rows = [(g, g, g % 4) for g in range(12)]
    bad_cls = scene(50, rows); bad_cls.loop_cls[5] = FEAT
    bad_cur = scene(51, rows); bad_cur.cur_cls[3] = -1
    bad_slot = scene(52, rows); bad_slot.lm[7] = LAND
    low_slot = scene(53, rows); low_slot.lm[2] = -2
    r, es = run_and_check(api, oracle, [scene(54, rows), bad_cls, bad_cur, scene(55, rows), bad_slot, low_slot, scene(56, rows)])
    assert [(len(e["pairs"]), e["count"], e["status"]) for e in es] == [(12, 12, OK), (0, 0, INVALID), (0, 0, INVALID), (12, 12, OK), (12, 0, INVALID),
                                                                        (12, 0, INVALID), (12, 12, OK)]


@gpu
def test_f32_rounding_of_landmark_positions(api, oracle):
    """cv::Point3f(pos(0), ...) rounds to nearest, ties to even: 1 + 2^-24 -> 1, 1 + 3 * 2^-25 -> 1 + 2^-23, -1e-40 -> a subnormal, 1e39 -> inf"""
    vals = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -25, -1e-40, 1e39, 1 + 2.0 ** -24 + 2.0 ** -50, 1 - 2.0 ** -25, -1e39, 3e-46, 0.1, -16777217.0, 1e-45, 65504.5]
    pos = np.zeros((LAND, 3)); pos[:12] = np.array([vals, vals[::-1], np.roll(vals, 5)]).T
    r, (e,) = run_and_check(api, oracle, [scene(60, [(g, g, g % 4) for g in range(12)], pos=pos)])
    assert e["count"] == 12 and e["p3"][:4, 0].view(np.uint32).tolist() == [0x3F800000, 0x3F800001, 0x800116C2, 0x7F800000]


@gpu
def test_both_matcher_paths(api, oracle):
    """12 items take the narrow matcher kernel, the same items in a batch of 17 the wide one (batch >= 16): item by item the same, and the reference's"""
    items = mixed_items()
    r12, es = run_and_check(api, oracle, items)
    assert sorted(set(e["status"] for e in es)) == [OK, FEW_PAIRS, FEW_POINTS]
    r17, _ = run_and_check(api, oracle, items + items[:5])
    for k in r12:
        assert np.array_equal(r12[k], r17[k][:12]) and np.array_equal(r17[k][12:], r12[k][:5]), k


@gpu
def test_landmark_stride(api, oracle):
    """landmark_stride 0 (one table for every item) and per-item tables holding the same rows"""
    items = [dup_item()] + landmark_items()
    table = np.random.default_rng(9).normal(0, 10, (LAND, 3))
    for it in items:
        it.pos = table
    own, _ = run_and_check(api, oracle, items)
    shared, _ = run_and_check(api, oracle, items, shared_table=True)
    assert all(np.array_equal(own[k], shared[k]) for k in own) and own["cnt"].tolist() == [13, 10, 9, 0]


@gpu
def test_limit_size(api, oracle):
    """cap 16384, every row present on both sides, about half kept: 2048 features x 8 levels, levels 0-5 within the limit, levels 6-7 (and every
    level of each third feature) at 50.  train_idx / dist against api.hamming_match_batch on the same buffers (tests/test_gpu_match_tri.py holds
    that against the oracle), the pair stage against the restatement on them.  cap 16385 is refused with nothing written."""
    cap, F = 16384, 2048
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, (F, 32), dtype=np.uint8)
    g = np.repeat(np.arange(F), 8); lvl = np.tile(np.arange(8), F)
    d = np.where((lvl < 6) & (g % 3 != 0), lvl * 6, 50)
    order = np.argsort(rng.random((cap, 256)), axis=1)
    bits = np.zeros((cap, 256), np.uint8); np.put_along_axis(bits, order, (np.arange(256)[None, :] < d[:, None]).astype(np.uint8), axis=1)
    f = (g * 5 + 3) % F
    shuffle = rng.permutation(cap)                                   # loop rows in no particular order
    it = Item((base[f] ^ np.packbits(bits, axis=1, bitorder="little"))[shuffle], g[shuffle], base[np.repeat(np.arange(F)[::-1], 8)], np.repeat(np.arange(F)[::-1], 8),
              rng.uniform(0, 1000, (F, 2)), np.where(np.arange(F) % 5 == 0, -1, np.arange(F) % LAND), rng.normal(0, 10, (LAND, 3)))
    bufs = Bufs(api, 1, cap=cap, feat_cap=F, out_cap=4096)
    bufs.load([it])
    ti, dist = bufs.t.zeros(cap, dtype=bufs.t.int32, device="cuda"), bufs.t.zeros(cap, dtype=bufs.t.int32, device="cuda")
    api.hamming_match_batch(bufs.ld.data_ptr(), bufs.nl.data_ptr(), bufs.cd.data_ptr(), bufs.nc.data_ptr(), 1, cap, ti.data_ptr(), dist.data_ptr())
    bufs.run()
    r = bufs.results()
    match = (ti.cpu().numpy(), dist.cpu().numpy())
    assert np.array_equal(match[1], d[shuffle])                      # the distances are the constructed ones
    e = expect(oracle, it, cap=cap, feat_cap=F, out_cap=4096, match=match)
    check(r, 0, e, cap, 4096)
    kept = int((match[1] <= 30).sum())
    assert 0.45 * cap < kept <= 0.5 * cap and len(e["pairs"]) == F - (F + 2) // 3 and e["status"] == OK and e["count"] == sum(1 for _, l in e["pairs"] if l % 5)
    bufs.clear()
    with pytest.raises(api.MyslamError) as err:
        bufs.run(cap=cap + 1)
    assert err.value.code == api.ERR_CAPACITY
    r = bufs.results()
    assert all((v == (FSENT if k in ("p3", "p2") else ISENT)).all() for k, v in r.items())


@gpu
def test_call_level_errors(api, oracle):
    bufs = Bufs(api, 1)
    bufs.load([dup_item()])
    for kw, code in ((dict(batch=-1), api.ERR_INVALID), (dict(cap=-1), api.ERR_INVALID)):
        with pytest.raises(api.MyslamError) as err:
            bufs.run(**kw)
        assert err.value.code == code
    for attr, value, code in (("out_cap", 0, api.ERR_INVALID), ("out_cap", 4097, api.ERR_CAPACITY), ("feat_cap", 65537, api.ERR_CAPACITY)):
        old = getattr(bufs, attr); setattr(bufs, attr, value)
        with pytest.raises(api.MyslamError) as err:
            bufs.run()
        setattr(bufs, attr, old)
        assert err.value.code == code
    with pytest.raises(api.MyslamError) as err:
        bufs.run(null_table=True)
    assert err.value.code == api.ERR_INVALID
    r = bufs.results()
    assert all((v == (FSENT if k in ("p3", "p2") else ISENT)).all() for k, v in r.items())       # nothing was enqueued


@gpu
def test_recorded(api, oracle):
    """the call recorded once into a StepGraph (matcher + pair kernel: two nodes) and replayed on rewritten inputs: the eager call's bits"""
    import torch
    sets = [[dup_item()] + landmark_items(), threshold_items() + [kept_item(257)]]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        bufs = Bufs(api, 4)
        eager = []
        for items in sets:
            bufs.load(items); bufs.run(stream=stream.cuda_stream)
            eager.append(bufs.results())
            for b, it in enumerate(items):
                check(eager[-1], b, expect(oracle, it))
        assert not all(np.array_equal(eager[0][k], eager[1][k]) for k in eager[0])
        g = api.StepGraph.record(stream.cuda_stream, [], lambda: bufs.run(stream=stream.cuda_stream))
        assert g.node_count() >= 2
        for items, want in zip(sets + sets[:1], eager + eager[:1]):
            bufs.load(items)
            g.launch(stream.cuda_stream)
            got = bufs.results()
            for k in want:
                assert np.array_equal(got[k], want[k]), k


@gpu
def test_chained_with_verification(api, synth):
    """loop_match_batch -> PnPSolver.verify_batch with no host step in between against the one-item path (api.hamming_match,
    api.match_feature_pairs, a host gather, verify_batch): status, pose bits, outlier flags and counts.  Four candidates made of
    synth.pnp_problem points, every point a feature with eight pyramid rows; every seventh loop feature has no map point; the candidate with
    eight pairs ends MYSLAM_VERIFY_FEW_MATCHES.  (A self-comparison: the oracle checks are the tests above.)"""
    import torch
    sizes, N = (200, 63, 120, 8), 200
    cap = 8 * N
    items, K = [], None
    for s, n in enumerate(sizes):
        pw, uv, K, _, _ = synth.pnp_problem(n, 0.3, 0.5, seed=20 + s)
        rng = np.random.default_rng(400 + s)
        base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        cls = np.repeat(np.arange(n), 8)
        loop_rows = rng.permutation(8 * n)
        lm = np.where(np.arange(n) % 7 == 6, -1, np.arange(n)[::-1]).astype(np.int32) if n > 8 else np.arange(n, dtype=np.int32)
        pos = np.zeros((N, 3)); pos[lm[lm >= 0]] = pw[lm >= 0].astype(np.float64) + 1e-9          # not representable in f32: the cast rounds
        items.append(Item(np.stack([_flip(base[f], int(rng.integers(0, 12)), rng) for f in cls[loop_rows]]), cls[loop_rows],
                          np.stack([_flip(base[f], int(rng.integers(0, 4)), rng) for f in cls]), cls, uv, lm, pos))
    B = len(items)
    bufs = Bufs(api, B, cap=cap, feat_cap=N, out_cap=N, landmark_cap=N)
    bufs.load(items)
    solver = api.PnPSolver(B, N, 100)
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device="cuda")

    def verify(p3, p2, cnt):
        pose, flag, ninl, st = z(B, 7, dt=torch.float64), z(B, N, dt=torch.uint8), z(B, dt=torch.int32), z(B, dt=torch.int32)
        pose.fill_(0.25); flag.fill_(255); ninl.fill_(ISENT); st.fill_(ISENT)
        solver.verify_batch(p3.data_ptr(), p2.data_ptr(), cnt.data_ptr(), B, K, pose.data_ptr(), flag.data_ptr(), ninl.data_ptr(), st.data_ptr())
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (pose, flag, ninl, st)]

    bufs.run()
    new = verify(bufs.out["p3"], bufs.out["p2"], bufs.out["cnt"])
    # the one-item path
    lk = np.zeros(cap, api.KP_DTYPE); ck = np.zeros(cap, api.KP_DTYPE)
    p3 = np.full((B, N, 3), np.nan, np.float32); p2 = np.full((B, N, 2), np.nan, np.float32); cnt = np.zeros(B, np.int32)
    for b, it in enumerate(items):
        n = len(it.loop_cls)
        ti, dist = api.hamming_match(it.loop_desc, it.cur_desc)
        lk["class_id"][:n] = it.loop_cls; ck["class_id"][:n] = it.cur_cls
        pairs = api.match_feature_pairs(ti, dist, lk[:n], ck[:n])
        if len(pairs) >= 10:
            valid = [(c, l) for c, l in pairs if it.lm[l] != -1]
            cnt[b] = len(valid)
            p3[b, :cnt[b]] = np.array([it.pos[it.lm[l]] for _, l in valid], np.float32).reshape(-1, 3)
            p2[b, :cnt[b]] = np.array([it.xy[c] for c, _ in valid], np.float32).reshape(-1, 2)
    r = bufs.results()
    assert r["cnt"].tolist() == cnt.tolist() == [172, 54, 103, 0] and r["np"].tolist() == [200, 63, 120, 8]
    assert r["st"].tolist() == [OK, OK, OK, FEW_PAIRS]
    old = verify(*(torch.from_numpy(x).cuda() for x in (p3, p2, cnt)))
    for a, b_ in zip(new, old):
        assert np.array_equal(a, b_)
    assert new[3].tolist() == [api.VERIFY_CONFIRMED] * 3 + [api.VERIFY_FEW_MATCHES] and (new[2][:3] >= 10).all()
