"""The loop-database scan kernels of csrc/lcddb.hip against tests/lcddb_scan_ref.py (plain numpy / Python loops, f64 scores): k_db_scan (f32 GEMV, fewer than 32
queries), k_db_scan_bf16x6 (matrix-core GEMM on three bf16 pieces per float, six products, from 32 queries), k_db_reduce and the pack / merge kernels.

Every case runs through BOTH scan kernels: the queries in calls of at most 31, and in one call padded with copies to at least 32.  Parts a to f feed
constructed inputs whose scores are exact in every f32 summation order (tests/test_lcddb_scan_ref.py asserts what each input is made of), so every assertion
there is bit or integer equality of whole output arrays.  Only the accuracy test carries a bar, computed in the test from the oracle's own f32 loop.

Out of scope: +-Inf descriptors.  A descriptor is the network output divided by its own L2 norm; an infinite entry makes the norm infinite and the entry
Inf / Inf = NaN, so Inf cannot reach the database, NaN can (and is tested)."""
import numpy as np
import pytest

import lcddb_scan_ref as R

pytestmark = pytest.mark.gpu
THR = R.THR


class _Dev:
    """a database on the device + the query entry points, results as numpy arrays"""

    def __init__(self, api, db, ids, capacity=None):
        import torch
        self.api, self.torch = api, torch
        self.ids = np.ascontiguousarray(ids, np.uint64)
        self.D = api.LoopDatabase(capacity or max(1, len(self.ids)))
        self.rows = torch.from_numpy(np.ascontiguousarray(db, np.float32)).cuda()
        self.D.append_batch(self.ids, self.rows.data_ptr(), len(self.ids))
        assert len(self.D) == len(self.ids)

    def _q(self, q):
        return self.torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()

    def batch(self, q, cur, thr):
        t, nq = self.torch, len(q)
        dq = self._q(q)
        b = t.full((nq,), -7, dtype=t.int64, device="cuda"); m = t.full((nq,), -7.0, device="cuda"); c = t.full((nq,), -7, dtype=t.int32, device="cuda")
        self.D.query_batch(dq.data_ptr(), cur, nq, b.data_ptr(), m.data_ptr(), c.data_ptr(), thr_low=float(thr))
        t.cuda.synchronize()
        return b.cpu().numpy().view(np.uint64), m.cpu().numpy(), c.cpu().numpy()

    def _records(self, fn, dtype, q, cur, thr):
        t, nq = self.torch, len(q)
        dq = self._q(q)
        rec = t.full((nq * dtype.itemsize,), 0xAB, dtype=t.uint8, device="cuda")
        fn(dq.data_ptr(), cur, nq, rec.data_ptr(), thr_low=float(thr))
        t.cuda.synchronize()
        return rec.cpu().numpy().view(dtype)

    def sharded(self, q, cur, thr):
        return self._records(self.D.query_batch_sharded, self.api.CAND_DTYPE, q, cur, thr)

    def owned(self, q, cur, thr):
        return self._records(self.D.query_batch_owned, self.api.OWNED_DTYPE, q, cur, thr)


def _paths(nq):
    """index lists of the calls that put nq queries through each kernel: at most 31 per call (GEMV), and padded with copies to 32 or more (GEMM)"""
    return {"gemv": [np.arange(a, min(a + 31, nq)) for a in range(0, nq, 31)], "gemm": [np.arange(max(nq, 32)) % nq]}


def _through(fn, q, cur, thr, calls):
    outs = [fn(q[ix], cur[ix], thr) for ix in calls]
    ix = np.concatenate(calls)
    if isinstance(outs[0], tuple):
        return ix, tuple(np.concatenate([o[k] for o in outs]) for k in range(3))
    return ix, np.concatenate(outs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, exp, what):
    """bit equality of arrays (or tuples of arrays, or record arrays)"""
    if isinstance(got, tuple):
        for k, (g, e) in enumerate(zip(got, exp)):
            _same(g, e, what + (("best_id", "max_score", "cnt")[k],))
        return
    if got.dtype.names:
        for f in got.dtype.names:
            _same(np.ascontiguousarray(got[f]), np.ascontiguousarray(exp[f]), what + (f,))
        return
    g, e = _bits(got), _bits(np.asarray(exp, got.dtype))
    bad = np.nonzero(g != e)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), "got", got[bad[0]], "expected", exp[bad[0]], f"{bad.size} of {g.size} differ")


def _expected(api, S, ids, cur, thr):
    nq = S.shape[1]
    plain = R.scan_many(S, ids, cur, thr)
    shard = np.array([R.shard_record(S[:, i], ids, cur[i], thr) for i in range(nq)], dtype=api.CAND_DTYPE)
    owned = np.array([R.owned_record(S[:, i], ids, cur[i], thr) for i in range(nq)], dtype=api.OWNED_DTYPE)
    return plain, shard, owned


def _check(api, dev, S, q, cur, thr=THR, tag="", single=8, natural=False):
    """every entry point, both kernels, whole output arrays against the restatement; returns the expected (plain, sharded, owned) results"""
    cur = np.ascontiguousarray(cur, np.uint64)
    q = np.ascontiguousarray(q, np.float32)
    exp = _expected(api, S, dev.ids, cur, thr)
    paths = _paths(len(q))
    if natural:
        paths["as_given"] = [np.arange(len(q))]
    for kernel, calls in paths.items():
        for name, fn, e in (("query_batch", dev.batch, exp[0]), ("query_batch_sharded", dev.sharded, exp[1]), ("query_batch_owned", dev.owned, exp[2])):
            ix, got = _through(fn, q, cur, thr, calls)
            _same(got, tuple(x[ix] for x in e) if isinstance(e, tuple) else e[ix], (tag, kernel, name))
    for i in range(min(single, len(q))):                                 # the one-query entry point
        got = dev.D.query(q[i], int(cur[i]), float(thr))
        want = (int(exp[0][0][i]), float(exp[0][1][i]), int(exp[0][2][i]))
        assert got == want and np.signbit(got[1]) == np.signbit(want[1]), (tag, "query", i, got, want)
    return exp


def _ids(n):
    return (100 + 30 * np.arange(n)).astype(np.uint64)


def _above(ids, nq):
    return np.full(nq, int(ids[-1]) + 20, np.uint64)


# ---- a. exact scores --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_hot_rows", "one_hot_queries"])
def test_one_hot_scores_are_bit_exact(api, case):
    """score = the one entry a one-hot vector picks, for every k of the sweep (GEMV lane and tail boundaries, GEMM k halves, the half-empty last stage), entries
    of 2^-20 .. 2^20 and both signs: max_score is that f32 bit for bit, best_id and cnt exact"""
    db, q = R.one_hot_rows_case() if case == "one_hot_rows" else R.one_hot_queries_case()
    assert R.one_term_ok(db, q)
    S = R.exact32(R.scores64(db, q)[0])
    ids = _ids(len(db)); dev = _Dev(api, db, ids)
    exp = _check(api, dev, S, q, _above(ids, len(q)), tag=case, single=len(q))
    assert (exp[0][1] >= 1).all() and len(set(exp[0][0].tolist())) > 5
    if case == "one_hot_rows":
        assert exp[0][0].tolist() == ids[:len(q)].tolist()                # query j's answer is the row that reads column ONE_HOT_K[j]
    cur = ids[(np.arange(len(q)) * 5 + 3) % len(ids)] + np.uint64(7)      # every query its own limit
    _check(api, dev, S, q, cur, tag=case + " limits")
    _check(api, dev, S, q, _above(ids, len(q)), thr=np.float32(-3.0), tag=case + " negative thr_low")


# ---- b. each of the six products ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.product_cases()))
def test_each_split_product_reaches_the_score(api, name):
    """N terms a * q on a 2^-g grid, spread over both k halves, many stages and the tail: the score N * a * q is exact in any f32 order, and it is wrong on the
    GEMM as soon as one of the products named in product_cases() is missing or pairs the wrong pieces (shown on the CPU in test_lcddb_scan_ref.py)"""
    row, qv, n, g, need = R.product_cases()[name]
    rows = (2, 45, 100, 131)                                              # several lanes, both wave rows, a second block
    db = np.zeros((140, R.DIM), np.float32); db[list(rows)] = row
    db[7] = row / 2; db[77] = -row                                         # exact too: a lower and a negative score
    q = np.stack([qv, qv / 4, -qv])
    assert R.pairs_exact(db, q)
    S64 = R.scores64(db, q)[0]
    S = R.exact32(S64)
    assert S64[rows[0], 0] == n * float(row.max()) * float(qv.max()) == R.six_product_value(row, qv)
    ids = _ids(len(db)); dev = _Dev(api, db, ids)
    exp = _check(api, dev, S, q, _above(ids, 3), thr=np.float32(n), tag=name)
    assert exp[0][0].tolist() == [ids[2], ids[2], ids[77]] and float(exp[0][1][0]) == S64[2, 0] and exp[0][2].tolist() == [4, 0, 1]
    for r in rows:                                                        # the same value from every position: each row alone in front of the limit
        one = np.zeros_like(db); one[r] = row
        _check(api, _Dev(api, one, ids), R.exact32(R.scores64(one, q)[0]), q, _above(ids, 3), thr=np.float32(n), tag=(name, r), single=1)


# ---- c. thresholds ------------------------------------------------------------------------------------------------------------------
def test_thresholds_are_strict(api):
    """scores of exactly thr_low, its two f32 neighbours, 0, -0.0 and negatives: only the neighbour above counts; a database with nothing above 0 answers
    (0, 0.0, cnt); a negative thr_low counts rows while the best stays 0"""
    db, q, V = R.threshold_case()
    S = R.exact32(R.scores64(db, q)[0])
    ids = _ids(len(db)); dev = _Dev(api, db, ids)
    up = np.nextafter(THR, np.float32(np.inf))
    e = _check(api, dev, S, q, _above(ids, 3), tag="thr")[0]
    assert e[2].tolist() == [1, 0, 1] and e[1].tolist() == [up, 0, up] and e[0][1] == 0
    e = _check(api, dev, S, q, _above(ids, 3), thr=np.float32(-0.5), tag="negative thr")[0]
    assert e[0][1] == 0 and e[1][1] == 0 and e[2][1] == int((V[:, 1] > -0.5).sum()) > 30
    e = _check(api, dev, S, q, _above(ids, 3), thr=np.float32(0.0), tag="thr 0")[0]      # -0.0 and 0.0 are not above 0
    assert e[2].tolist() == [int((V[:, i] > 0).sum()) for i in range(3)] and e[2][1] == 0
    for thr in (up, np.nextafter(THR, np.float32(-np.inf))):
        _check(api, dev, S, q, _above(ids, 3), thr=thr, tag=("thr", float(thr)))
    cur = np.array([ids[6], ids[3], ids[3]], np.uint64)                   # limits in front of the only counted row
    e = _check(api, dev, S, q, cur, tag="thr limits")[0]
    assert e[2].tolist() == [0, 0, 0]


# ---- d. ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,far", [(2049, (0, 2048)), (2049, (33, 2048)), (8193, (5, 8192)), (8193, (130, 8192))])
def test_equal_scores_keep_the_lowest_id(api, n, far):
    """bit-identical rows inside ONE matrix, the query equal to them: the lowest id wins wherever the pair sits — in one lane, across the k-half lanes, the two
    wave rows, two blocks, and 64 blocks apart (65 blocks: a lane of k_db_reduce holds two partials; with the lower copy in block 1 the higher block sits in
    the lower lane).  Three copies with limits between them: of the copies a scan sees, the lowest wins — for the suffix of an owned shard the middle one."""
    groups = R.tie_groups(n, *far)
    db, q = R.tie_case(n, groups)
    ids = _ids(n); dev = _Dev(api, db, ids)
    g3 = groups[-1]; tri = len(groups) - 1; fg = len(groups) - 2
    extra = [(tri, ids[g3[1]]), (tri, ids[g3[2]]), (tri, ids[g3[1]] - np.uint64(5)), (tri, ids[g3[0]]), (tri, ids[g3[2]] - np.uint64(5)),
             (fg, ids[far[1]]), (fg, ids[far[0]] + np.uint64(25)), (0, ids[groups[0][1]]), (3, ids[groups[3][1]] - np.uint64(5))]
    qq = np.concatenate([q, q[[g for g, _ in extra]]])
    cur = np.concatenate([_above(ids, len(q)), np.array([c for _, c in extra], np.uint64)])
    S = R.exact32(R.scores64(db, qq)[0])
    plain, shard, owned = _check(api, dev, S, qq, cur, tag=(n, far), single=len(qq))
    assert plain[0][:len(q)].tolist() == [int(ids[min(rows)]) for rows in groups] and (plain[1][:len(q)] == 1.25).all()
    k = len(q)
    assert plain[0][k] == plain[0][k + 1] == ids[g3[0]] and plain[1][k + 3] == 0.5          # limit behind the first / second copy; in front of all three
    assert owned["pre_best_id"][k + 2] == ids[g3[0]] and owned["suf_best_id"][k + 2] == ids[g3[1]] and owned["suf_max_score"][k + 2] == 1.25
    assert owned["suf_best_id"][k + 4] == ids[g3[2]]
    assert plain[0][k + 5] == ids[far[0]] and owned["suf_best_id"][k + 6] == ids[far[1]] and owned["suf_max_score"][k + 6] == 1.25


# ---- e. limits on boundaries -------------------------------------------------------------------------------------------------------
NQS = (1, 2, 31, 32, 33, 127, 128, 129, 257)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 257])
def test_row_limits_on_wave_tile_and_block_boundaries(api, n):
    """the best row of the matrix just outside a query's limit, the best visible row just inside, limits on 0, 1, 4, 8, 31 .. 33, 64, 127 .. 129 and past the
    end, different limits (0 among them) side by side in one call, for every count of rows and of queries next to a tile edge"""
    lim = [p for p in R.LIMITS if p <= n] + [n + 1]
    for nq in NQS:
        limits = [lim[(i * 7 + nq) % len(lim)] for i in range(nq)]
        if nq >= len(lim):
            limits[:len(lim)] = lim
        db, ids, q, cur = R.limit_case(n, limits)
        if nq == NQS[0]:
            dev = _Dev(api, db, ids, capacity=n + 3)
        S = R.exact32(R.scores64(db, q)[0])
        e = _check(api, dev, S, q, cur, tag=(n, nq), single=2, natural=True)[0]
        for i, p in enumerate(limits):
            if p <= n:
                assert (e[0][i], e[1][i]) == ((ids[p - 1], 2) if p >= 1 else (0, 0))


def test_owned_shard_ranges_on_boundaries(api):
    """an owned shard reports the rows below the cut-off window and the rows above cur separately: the first suffix row on every boundary with a better row
    just in front of it, equal scores on both sides, a query without a suffix beside queries with one, and the last suffix row on every boundary through
    the window that wraps around 2^64 (cur < 19, ids at 2^64 - k)"""
    db, ids, q, cur = R.owned_start_case()
    dev = _Dev(api, db, ids)
    S = R.exact32(R.scores64(db, q)[0])
    plain, shard, owned = _check(api, dev, S, q, cur, tag="owned start", natural=True)
    for j, t in enumerate(R.LIMITS):
        a, b, c = 3 * j, 3 * j + 1, 3 * j + 2
        assert owned["suf_best_id"][a] == ids[t] and owned["suf_max_score"][a] == 2 and owned["pre_best_id"][a] == (ids[t - 1] if t else 0)
        assert owned["suf_best_id"][b] == ids[t] and owned["suf_max_score"][b] == 4 and owned["pre_cnt"][c] < 0 <= owned["pre_cnt"][a]
        assert owned["suf_max_score"][c] < 2
        one = R.merge_owned([[tuple(x) for x in owned[[a, b, c]]]])
        assert one[0].tolist() == [int(ids[t - 1]) if t else int(ids[t])] * 2 + [int(ids[t - 1]) if t else 0]      # equal scores: the prefix id is kept
    assert owned[-1]["suf_cnt"] == 0 and owned[-1]["suf_max_score"] == 0 and owned[-1]["pre_cnt"] >= 0
    for t0, small in ((0, ()), (31, (3, 10)), (64, ()), (127, ())):
        db, ids, q, cur = R.owned_wrap_case(t0, small)
        dev = _Dev(api, db, ids)
        S = R.exact32(R.scores64(db, q)[0])
        plain, shard, owned = _check(api, dev, S, q, cur, tag=("owned wrap", t0), single=21)
        for c in range(19):
            if not small:
                assert owned["suf_best_id"][c] == (ids[t0 + c - 1] if t0 + c else 0) and owned["suf_max_score"][c] == (2 if t0 + c else 0)
                assert plain[0][c] == owned["suf_best_id"][c]
            assert owned["pre_max_score"][c] == 0 and owned["suf_max_score"][c] < 4


def _merge_both(api, torch, gathered, dtype, device_fn, host_fn):
    ns, nq = gathered.shape
    d = torch.from_numpy(gathered.view(np.uint8).reshape(-1).copy()).cuda()
    b = torch.zeros(nq, dtype=torch.int64, device="cuda"); m = torch.zeros(nq, device="cuda"); c = torch.zeros(nq, dtype=torch.int32, device="cuda")
    device_fn(d.data_ptr(), ns, nq, b.data_ptr(), m.data_ptr(), c.data_ptr())
    torch.cuda.synchronize()
    return (b.cpu().numpy().view(np.uint64), m.cpu().numpy(), c.cpu().numpy()), host_fn(gathered)


@pytest.mark.parametrize("kernel", ["gemv", "gemm"])
def test_shard_records_merge_to_one_scan(api, kernel):
    """the whole map cut into id ranges (cuts on tile edges) and dealt out by arrival (2, 3 and 8 shards): the records of every shard are what the restatement
    says, and the device merge and the host merge of them both equal ONE scan of the whole matrix — ties across shards, breaks in every shard, the wrap"""
    import torch
    db, ids, q, cur = R.whole_map_case()
    n = len(ids)
    S = R.exact32(R.scores64(db, q)[0])
    whole = R.scan_many(S, ids, cur)
    calls = _paths(len(q))[kernel]

    def records(parts, fn_name, dtype, ref_fn):
        out = []
        for rows in parts:
            dev = _Dev(api, db[rows], ids[rows], capacity=len(rows) + 5)
            ix, got = _through(getattr(dev, fn_name), q, cur, THR, calls)
            exp = np.array([ref_fn(S[rows, i], ids[rows], cur[i]) for i in range(len(q))], dtype=dtype)
            _same(got, exp[ix], (kernel, fn_name, len(parts), int(rows[0])))
            out.append(got[:len(q)])
        return np.stack(out)

    for cuts in ([0, 128, 161, n], [0, 1, 33, 257, n]):
        g = records([np.arange(a, b) for a, b in zip(cuts[:-1], cuts[1:])], "sharded", api.CAND_DTYPE, R.shard_record)
        for got in _merge_both(api, torch, g, api.CAND_DTYPE, api.lcd_merge_candidates_device, api.lcd_merge_candidates):
            _same(got, whole, (kernel, "ranges", tuple(cuts)))
    for ns in (2, 3, 8):
        g = records([np.arange(s, n, ns) for s in range(ns)][::-1], "owned", api.OWNED_DTYPE, R.owned_record)
        for got in _merge_both(api, torch, g, api.OWNED_DTYPE, api.lcd_merge_owned_candidates_device, api.lcd_merge_owned_candidates):
            _same(got, whole, (kernel, "owned", ns))


# ---- f. NaN --------------------------------------------------------------------------------------------------------------------------
def test_nan_rows_and_queries_stay_where_they_are(api):
    """one NaN in a row takes that row out of every scan, one NaN in a query makes that query answer (0, 0.0, 0); their neighbours in the same tile are
    untouched.  Row 0 and query 0 are among them: the GEMM reads row 0 / query 0 for every row and query beyond the end of a partly filled tile.  The
    handle's capacity (77) is no multiple of 32 or 128 and holds more rows than are appended"""
    n, nq = 70, 33
    db, q, cols = R.graded(n, nq)
    free = [c for c in range(R.DIM) if c not in set(cols.tolist())]
    assert R.one_term_ok(db, q)
    nan_rows = {0: free[0], 37: 9, 50: 1063, 64: free[5], 69: 1040}
    nan_q = {0: 12, 20: 1060, 32: int(cols[3])}
    for r, c in nan_rows.items():
        db[r, c] = np.nan
    for i, c in nan_q.items():
        q[i, c] = np.nan
    S = R.exact32(R.scores64(db, q)[0])
    assert np.isnan(S[list(nan_rows)]).all() and np.isnan(S[:, list(nan_q)]).all() and np.isnan(S).sum() == len(nan_rows) * nq + len(nan_q) * (n - len(nan_rows))
    ids = _ids(n)
    dev = _Dev(api, db, ids, capacity=77)
    assert dev.D.capacity() % 128 != 0 and dev.D.capacity() > n
    keep = [r for r in range(n) if r not in nan_rows]
    limited = ids[np.array(keep)[(np.arange(nq) * 11 + 1) % len(keep)]] + np.uint64(3)      # the row inside the window is never a NaN row
    for cur in (_above(ids, nq), limited):
        e = _check(api, dev, S, q, cur, tag="nan", natural=True, single=nq)[0]
        for i in nan_q:
            assert (e[0][i], e[1][i], e[2][i]) == (0, 0, 0) and not np.signbit(e[1][i])
        clean = R.scan_many(np.nan_to_num(S[keep]), ids[keep], cur)       # the same answers as from a database without the NaN rows
        ok = [i for i in range(nq) if i not in nan_q]
        assert all(np.array_equal(a[ok], b[ok]) for a, b in zip(e, clean)) and (cur is limited or (e[1][ok] > 0).all())


# ---- g. accuracy against f64 on the model's ranges ---------------------------------------------------------------------------------
def _accuracy_set(kind):
    rng = np.random.default_rng({"gauss": 71, "relu": 72, "wide": 73}[kind])
    x = rng.standard_normal((340, R.DIM))
    if kind == "relu":
        x = np.maximum(x - 0.5, 0.0)                                      # the post-ReLU shape: non-negative, about 70 % exact zeros
    if kind == "wide":
        x = x * np.exp2(rng.integers(-12, 13, x.shape))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(x[:300]), np.ascontiguousarray(x[300:])


@pytest.mark.parametrize("kind", ["gauss", "relu", "wide"])
def test_scores_are_as_accurate_as_the_reference_loop(api, oracle, kind):
    """e = |score - f64| / (u * A), u = 2^-24, A = |row| . |query|, for each of 300 x 40 pairs, on both kernels and for the oracle's own f32 loop
    (orc_lcd_score): max e(device) <= 4 * max e(oracle loop) per set and kernel.  The factor 4 is the issue's allowance for the matrix core's undocumented
    summation order; it was fixed before any run on hardware.

    The scan returns one maximum per query, so every row is read alone: it sits at a row of its own in a matrix of zero rows (positions wander over
    lanes, wave rows and two blocks), and the sign of each query is chosen so that the pair's score is positive (negation is exact in every step of both
    kernels).  The same call checks scaling: the row times 2^8 further up, the queries times 2^-5, must give the same bits times 2^3.

    Measured on an MI355X (max e: GEMV / GEMM / oracle loop): gauss 0.37 / 3.08 / 4.10, relu 2.35 / 16.96 / 10.33, wide 3.44 / 20.59 / 20.19.  With the
    mm product removed from the GEMM the relu and wide sets miss the bar."""
    import torch
    db, q = _accuracy_set(kind)
    S64, A = R.scores64(db, q)
    assert (A > 0).all() and (S64 != 0).all()
    sign = np.where(S64 < 0, -1.0, 1.0).astype(np.float32)               # [rows, queries]
    ids = _ids(200)
    zeros = torch.zeros(200, R.DIM, device="cuda")
    nq = len(q)
    calls = _paths(2 * nq)
    got = {k: np.zeros((len(db), 2 * nq), np.float32) for k in calls}
    for r in range(len(db)):
        a = (r * 29) % 160; b = a + 1 + r % 37
        D = api.LoopDatabase(200)
        pair = torch.from_numpy(np.stack([db[r], db[r] * np.float32(256)])).cuda()
        for first, src, cnt in ((0, zeros.data_ptr(), a), (a, pair.data_ptr(), 1), (a + 1, zeros.data_ptr(), b - a - 1), (b, pair.data_ptr() + R.DIM * 4, 1)):
            if cnt:
                D.append_batch(ids[first:first + cnt], src, cnt)
        qs = q * sign[r][:, None]
        qq = np.concatenate([qs, qs * np.float32(2.0 ** -5)])
        cur = np.concatenate([np.full(nq, ids[a + 1], np.uint64), np.full(nq, ids[b] + np.uint64(25), np.uint64)])
        dq = torch.from_numpy(qq).cuda()
        for k, cl in calls.items():
            for ix in cl:
                m = torch.zeros(len(ix), device="cuda"); bb = torch.zeros(len(ix), dtype=torch.int64, device="cuda"); c = torch.zeros(len(ix), dtype=torch.int32, device="cuda")
                sel = dq if len(ix) == 2 * nq and ix[0] == 0 else dq[torch.from_numpy(ix).cuda()].contiguous()
                D.query_batch(sel.data_ptr(), cur[ix], len(ix), bb.data_ptr(), m.data_ptr(), c.data_ptr(), thr_low=0.0)
                torch.cuda.synchronize()
                got[k][r, ix] = m.cpu().numpy()
                bid = bb.cpu().numpy().view(np.uint64)
                assert set(bid.tolist()) <= {0, int(ids[a]), int(ids[b])}
    ref_abs = np.abs(S64)
    e_or = np.zeros_like(S64)
    for r in range(len(db)):
        for i in range(nq):
            e_or[r, i] = abs(float(oracle.lcd_score(q[i] * sign[r, i], db[r])) - ref_abs[r, i])
    e_or = e_or / (R.U * A)
    msg = {}
    for k in calls:
        plain, scaled = got[k][:, :nq], got[k][:, nq:]
        assert np.array_equal((plain * np.float32(8)).view(np.uint32), scaled.view(np.uint32)), (kind, k, "scaling by 2^8 and 2^-5 is not exact")
        msg[k] = float((np.abs(plain.astype(np.float64) - ref_abs) / (R.U * A)).max())
    line = f"{kind}: max e gemv {msg['gemv']:.2f}, gemm {msg['gemm']:.2f}, oracle loop {e_or.max():.2f} (bar {4 * e_or.max():.2f})"
    print(line)
    assert msg["gemv"] <= 4 * e_or.max() and msg["gemm"] <= 4 * e_or.max(), line
