"""The loop database bank (csrc/lcd_bank.hip, api.LoopDatabaseBank) on the device against tests/lcd_bank_ref.py.

Parts 1 to 7 feed constructed inputs — one-hot rows, queries from lcddb_scan_ref — whose scores are exact in every f32 summation order, so every
assertion there is equality of whole output arrays (floats by their bits); every output buffer is pre-filled with a sentinel.  Wherever the allocation
is small the whole of it (rows, ids, counts, bytes behind the counts included) is read back through view() and compared with a host mirror after
every call.  Only the accuracy test carries a bar, the error of the oracle's own f32 loop on the same pairs."""
import os
import subprocess

import numpy as np
import pytest

import lcd_bank_ref as B
import lcddb_scan_ref as R

pytestmark = pytest.mark.gpu
DIM = R.DIM
SENT_I, SENT_F = -7, -7.0
CANARY_ID = 0xC0FFEE0000


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, exp, what):
    names = ("best_id", "max_score", "cnt", "best_row", "status")
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        g, e = _bits(g), _bits(np.asarray(e, g.dtype))
        assert g.shape == e.shape, (what, names[k], g.shape, e.shape)
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (what, names[k], "first difference at item", int(bad[0]), "got", got[k][bad[0]], "expected", exp[k][bad[0]], f"{bad.size} of {g.size} differ")


class Pair:
    """the device bank and the model, fed the same calls; `mirror` = what the whole allocation must hold"""

    def __init__(self, api, S, cap, stream=None, mirror=True):
        import torch
        self.api, self.torch, self.S, self.cap = api, torch, S, cap
        self.dev = api.LoopDatabaseBank(S, cap, stream)
        self.ref = B.Bank(S, cap)
        self.m_rows = np.zeros((S, cap, DIM), np.float32) if mirror else None
        self.m_ids = np.zeros((S, cap), np.uint64)

    def load(self, s, ids, rows):
        ids = np.ascontiguousarray(ids, np.uint64); rows = np.ascontiguousarray(rows, np.float32).reshape(len(ids), DIM)
        self.dev.load(s, ids, rows); self.ref.load(s, ids, rows)
        if self.m_rows is not None:
            self.m_rows[s, :len(ids)] = rows
        self.m_ids[s, :len(ids)] = ids

    def canaries(self):
        """every slot of every stream holds a row of 7.5s and a canary id; the streams are empty afterwards"""
        ids = CANARY_ID + np.arange(self.cap, dtype=np.uint64)
        for s in range(self.S):
            self.load(s, ids, np.full((self.cap, DIM), 7.5, np.float32))
            self.load(s, [], np.zeros((0, DIM), np.float32))

    def outputs(self):
        t = self.torch
        S = self.S
        return [t.full((S,), SENT_I, dtype=t.int64, device="cuda"), t.full((S,), SENT_F, device="cuda"), t.full((S,), SENT_I, dtype=t.int32, device="cuda"),
                t.full((S,), SENT_I, dtype=t.int32, device="cuda"), t.full((S,), SENT_I, dtype=t.int32, device="cuda")]

    @staticmethod
    def fetch(out):
        return (out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy(), out[4].cpu().numpy())

    def query(self, q, cur, active=None, thr=R.THR, min_size=0, what=""):
        """one call on sentinel-filled outputs, compared whole with the model; -> the expected arrays"""
        q = np.ascontiguousarray(q, np.float32); cur = np.ascontiguousarray(cur, np.uint64)
        dq, dc = _t(q), _t(cur)
        da = None if active is None else _t(np.asarray(active, np.int32))
        out = self.outputs()
        self.dev.query_batch(dq.data_ptr(), dc.data_ptr(), 0 if da is None else da.data_ptr(), *[o.data_ptr() for o in out], thr_low=float(thr), min_size=min_size)
        self.torch.cuda.synchronize()
        exp = B.as_arrays(self.ref.query(q, cur, active, thr, min_size))
        _same(self.fetch(out), exp, what)
        return exp

    def append(self, descr, ids, add=None, what=""):
        descr = np.ascontiguousarray(descr, np.float32); ids = np.ascontiguousarray(ids, np.uint64)
        dd, di = _t(descr), _t(ids)
        da = None if add is None else _t(np.asarray(add, np.int32))
        st = self.torch.full((self.S,), SENT_I, dtype=self.torch.int32, device="cuda")
        self.dev.append_batch(dd.data_ptr(), di.data_ptr(), 0 if da is None else da.data_ptr(), st.data_ptr())
        self.torch.cuda.synchronize()
        n0 = self.ref.sizes()
        want = self.ref.append(descr, ids, add)
        self.note_added(want, n0, descr, ids)
        got = st.cpu().numpy().tolist()
        assert got == want, (what, got, want)
        return want

    def note_added(self, status, n0, descr, ids):
        for s, w in enumerate(status):
            if w == B.ADDED:
                if self.m_rows is not None:
                    self.m_rows[s, n0[s]] = descr[s]
                self.m_ids[s, n0[s]] = ids[s]

    def clear(self, flags):
        d = _t(np.asarray(flags, np.int32))
        self.dev.clear_batch(d.data_ptr())
        self.torch.cuda.synchronize()
        self.ref.clear(flags)

    def check_view(self, what=""):
        """the whole allocation, bytes behind the counts included"""
        rows, ids, n = self.dev.read_view()
        assert n.tolist() == self.ref.sizes() == self.dev.sizes().tolist(), (what, n, self.ref.sizes())
        assert np.array_equal(ids, self.m_ids), what
        assert np.array_equal(rows.view(np.uint32), self.m_rows.view(np.uint32)), what

    def check_get(self):
        for s in range(self.S):
            ids, rows = self.dev.get(s)
            assert ids.tolist() == self.ref.ids[s], s
            want = np.stack(self.ref.rows[s]) if self.ref.rows[s] else np.zeros((0, DIM), np.float32)
            assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), s


def _free_cols(used, k):
    used = set(int(c) for c in used)
    return [c for c in range(DIM) if c not in used][:k]


# ---- 1. boundaries ----------------------------------------------------------------------------------------------------------------
def _counts(T, cap):
    return [0, 1, T - 1, T, T + 1, 2 * T, cap]


def _boundary_inputs(T, cap, ps):
    """per stream s the limit_case of limit ps[s] over cap rows; every row of stream t also holds 1.0 at the columns Y_u of the OTHER streams u, and query s holds 8.0
    at Y_s: every row of a neighbouring partition beats everything stream s may see"""
    S = len(ps)
    cols = R.spread_cols(cap)
    Y = _free_cols(cols, S)
    dbs, qs, curs, ids = [], [], [], None
    for s, p in enumerate(ps):
        db, ids, q, cur = R.limit_case(cap, [p])
        for u in range(S):
            if u != s:
                db[:, Y[u]] = 1.0
        q[0, Y[s]] = 8.0
        dbs.append(db); qs.append(q[0]); curs.append(cur[0])
    return dbs, ids, np.stack(qs), np.array(curs, np.uint64)


@pytest.mark.parametrize("how", ["count", "window"])
def test_limits_on_tile_boundaries_stay_inside_their_partition(api, how):
    """S = 3, rows_per_stream = two row tiles + 6, limits on 0, 1, tile - 1, tile, tile + 1, 2 tiles and the capacity, three different ones side by side in every
    rotation.  `count`: the stream HOLDS that many rows (the best row of the partition, score 4, lies in the slot right behind the count, left there by an
    earlier load); `window`: the stream is full and the cut-off window ends the scan there.  The rows of both neighbouring partitions score 8 or more."""
    T = api.LoopDatabaseBank.row_tile()
    assert T == api.lib().myslam_lcdbank_row_tile() and T >= 2
    S, cap = 3, 2 * T + 6
    counts = _counts(T, cap)
    p = Pair(api, S, cap)
    for k in range(len(counts)):
        ps = [counts[(k + 2 * s) % len(counts)] for s in range(S)]
        assert len(set(ps)) == S
        dbs, ids, q, cur = _boundary_inputs(T, cap, ps)
        for s in range(S):
            p.load(s, ids, dbs[s])
            if how == "count":
                p.load(s, ids[:ps[s]], dbs[s][:ps[s]])                         # rows ps[s] .. stay in memory behind the count
        if how == "count":
            cur = np.full(S, int(ids[-1]) + 25, np.uint64)
        p.check_view((how, ps))
        e = p.query(q, cur, min_size=-1, what=(how, ps))
        for s in range(S):
            want = (int(ids[ps[s] - 1]), 2.0, ps[s] - 1) if ps[s] >= 1 else (0, 0.0, -1)
            assert (int(e[0][s]), float(e[1][s]), int(e[3][s])) == want and e[4][s] == B.SCANNED, (how, ps, s)
        p.check_view((how, ps, "after"))


# ---- 2. ties and thresholds -------------------------------------------------------------------------------------------------------
def test_equal_scores_keep_the_lowest_row(api):
    """bit-identical rows inside one stream, the query equal to them: the lowest row wins wherever the pair sits — in one tile at every distance a wave split could
    put between them, in adjacent tiles, 64 tiles apart in ONE lane of the reduce, and 63 tiles apart with the higher tile in the LOWER lane.  Stream 1 holds the
    same rows and ends its scan at the second copy, and at the first (no copy seen: the background wins)."""
    T = api.LoopDatabaseBank.row_tile()
    offs = sorted({1, 2, 4, 8, 16, T // 2, T - 1, T, T + 1})
    groups = [[T * (2 * j + 1), T * (2 * j + 1) + off] for j, off in enumerate(offs)]
    base = T * (2 * len(offs) + 2)
    groups += [[base + 2, base + 64 * T + 2], [base + T + 3, base + 64 * T + 5], [base + 3 * T, base + 3 * T + 1, base + 4 * T + 8]]
    n = base + 65 * T
    db, q = R.tie_case(n, groups)
    ids = (100 + 30 * np.arange(n)).astype(np.uint64)
    p = Pair(api, 2, n + 6, mirror=False)
    p.load(0, ids, db); p.load(1, ids, db)
    for g, rows in enumerate(groups):
        qq = np.stack([q[g], q[g]])
        e = p.query(qq, [int(ids[-1]) + 25, int(ids[rows[1]])], what=("tie", rows))
        assert e[3].tolist() == [rows[0], rows[0]] and e[1].tolist() == [1.25, 1.25] and e[0][0] == ids[rows[0]], rows
        e = p.query(qq, [int(ids[rows[-1]]) + 7, int(ids[rows[0]]) + 19], what=("tie, limits", rows))
        assert e[3][0] == rows[0] and e[1][1] == 0.5 and e[3][1] == 0, rows               # background: e_BG rows score 0.5, row 0 is the first of them


@pytest.mark.parametrize("nan", [False, True])
def test_thresholds_are_strict_and_nan_is_nothing(api, nan):
    """scores of exactly thr_low, its two f32 neighbours, 0, -0.0 and negatives, with thr_low on each of the three values; then the same with a NaN in the
    rows that held the winners: a NaN row neither wins nor counts, its neighbours answer as before"""
    db, q, V = R.threshold_case()
    ids = (100 + 30 * np.arange(len(db))).astype(np.uint64)
    free = _free_cols(R.spread_cols(len(db)), 2)
    p = Pair(api, 3, len(db) + 3)
    dbs = [db.copy() for _ in range(3)]
    if nan:
        dbs[0][6, free[0]] = np.nan; dbs[2][3, free[1]] = np.nan; dbs[1][0, 0] = np.nan
        q = q.copy(); q[0, free[0]] = 1.0                                       # (NaN * 0 is NaN as well: either way the row's score is NaN)
    for s in range(3):
        p.load(s, ids, dbs[s])
    cur = np.full(3, int(ids[-1]) + 25, np.uint64)
    up, dn = np.nextafter(R.THR, np.float32(np.inf)), np.nextafter(R.THR, np.float32(-np.inf))
    e = p.query(q, cur, what="thr")
    if not nan:
        assert e[2].tolist() == [1, 0, 1] and e[1].tolist() == [up, 0, up] and e[0][1] == 0 and e[3][1] == -1
    else:
        assert e[2].tolist() == [0, 0, 0] and e[1].tolist() == [R.THR, 0, R.THR]
    for thr in (up, dn, np.float32(0.0), np.float32(-0.5)):
        p.query(q, cur, thr=thr, what=("thr", float(thr)))
    p.check_view("thr")


# ---- 3. gate, idle and statuses ----------------------------------------------------------------------------------------------------
def test_gate_idle_and_refusals_keep_every_byte(api):
    S, cap = 6, 6
    p = Pair(api, S, cap)
    p.canaries()
    db, q, cols = R.graded(cap, S)
    ids = (10 + 5 * np.arange(cap)).astype(np.uint64)
    n = [0, 2, 3, 6, 4, 3]
    for s in range(S):
        p.load(s, ids[:n[s]], db[:n[s]])
    p.check_view("loaded")
    cur = np.full(S, 1000, np.uint64)
    for min_size, active in ((2, None), (3, None), (2, [1, 1, 0, 1, 0, 1]), (0, [0] * S), (5, [1] * S), (6, None)):
        e = p.query(q, cur, active, min_size=min_size, what=("gate", min_size, active))
        for s in range(S):
            st = B.IDLE if active is not None and not active[s] else (B.GATED if n[s] <= min_size else B.SCANNED)
            assert e[4][s] == st, (min_size, active, s)
            if st != B.SCANNED:
                assert (e[0][s], e[1][s], e[2][s], e[3][s]) == (0, 0, 0, -1) and not np.signbit(e[1][s])
        p.check_view(("gate", min_size))
    new = R.one_hot(_free_cols(cols, S), 0.5)
    st = p.append(new, [1, 15, 19, 99, 26, 21], add=[1, 1, 1, 1, 1, 0], what="append")
    assert st == [B.ADDED, B.ERR_INVALID, B.ERR_INVALID, B.ERR_CAPACITY, B.ADDED, B.IDLE]      # empty: any id; equal; lower; full; above; not selected
    p.check_view("append")
    e = p.query(new * np.float32(4), cur, what="after append")           # a query behind the append sees the row
    assert e[3].tolist() == [0, -1, -1, -1, 4, -1] and e[1].tolist() == [1, 0, 0, 0, 1, 0]
    assert p.append(new, [2, 21, 21, 100, 27, 22], what="append all") == [B.ADDED] * 3 + [B.ERR_CAPACITY] + [B.ADDED] * 2
    p.check_view("append all")
    p.clear([0, 1, 0, 1, 0, 0])
    p.check_view("clear")                                                      # a clear moves the counts and nothing else
    assert p.ref.sizes() == [2, 0, 4, 0, 6, 4]
    assert p.append(new, [0, 0, 0, 0, 0, 0], add=[0, 1, 0, 1, 1, 0]) == [B.IDLE, B.ADDED, B.IDLE, B.ADDED, B.ERR_CAPACITY, B.IDLE]
    p.check_view("append after clear"); p.check_get()


def test_call_level_errors(api):
    import torch
    lib, INV, CAPA = api.lib(), api.ERR_INVALID, api.ERR_CAPACITY
    import ctypes as C
    h = C.c_void_p()
    assert lib.myslam_lcdbank_create(None, 1, 1) == INV and lib.myslam_lcdbank_create(C.byref(h), 0, 4) == INV
    assert lib.myslam_lcdbank_create(C.byref(h), 4, 0) == INV and lib.myslam_lcdbank_create(C.byref(h), 65536, 1) == CAPA and not h.value
    p = Pair(api, 2, 4)
    p.canaries()
    ids = np.array([3, 5, 9], np.uint64); rows = R.one_hot([1, 2, 3])
    p.load(1, ids, rows)
    code = lambda fn, *a: lib_call(api, fn, *a)
    assert code(p.dev.load, 1, [3, 3], rows[:2]) == INV and code(p.dev.load, 1, [4, 3], rows[:2]) == INV
    assert code(p.dev.load, 1, np.arange(5), R.one_hot(range(5))) == CAPA and code(p.dev.load, 2, ids, rows) == INV and code(p.dev.load, -1, ids, rows) == INV
    p.check_view("refused loads")
    q = torch.zeros(2 * DIM + 1, device="cuda"); u = torch.zeros(2, dtype=torch.int64, device="cuda"); i = torch.full((2,), SENT_I, dtype=torch.int32, device="cuda")
    good = [q.data_ptr(), u.data_ptr(), 0, u.data_ptr(), q.data_ptr(), i.data_ptr(), i.data_ptr(), i.data_ptr()]
    for k in (0, 1, 3, 4, 5, 6, 7):
        assert code(p.dev.query_batch, *(good[:k] + [0] + good[k + 1:])) == INV, k
    assert code(p.dev.query_batch, *([q.data_ptr() + 4] + good[1:])) == INV                  # the queries are read with 16-byte loads
    ga = [q.data_ptr(), u.data_ptr(), 0, i.data_ptr()]
    for k in (0, 1, 3):
        assert code(p.dev.append_batch, *(ga[:k] + [0] + ga[k + 1:])) == INV, k
    assert code(p.dev.clear_batch, 0) == INV
    assert lib.myslam_lcdbank_query_batch(None, *[C.c_void_p(x or None) for x in good[:3]], C.c_float(0.92), 0, *[C.c_void_p(x) for x in good[3:]]) == INV
    assert lib.myslam_lcdbank_sizes(p.dev._h, None) == INV and lib.myslam_lcdbank_destroy(None) == INV
    torch.cuda.synchronize()
    assert (i.cpu().numpy() == SENT_I).all()                                   # nothing was enqueued
    p.check_view("refused calls")
    assert api.LoopDatabaseBank.launches_per_query() <= 3


def lib_call(api, fn, *a):
    try:
        fn(*a)
        return 0
    except api.MyslamError as e:
        return e.code


# ---- 4. random histories -----------------------------------------------------------------------------------------------------------
def _history_step(rng, S, t, next_id, q_all):
    active = rng.integers(0, 4, S) > 0
    add = rng.random(S) < 0.8
    step = rng.integers(1, 4, S)
    ids = np.array([next_id[s] + int(step[s]) for s in range(S)], np.uint64)
    cols = (np.arange(S) * 37 + t * 101 + 5) % DIM
    descr = R.one_hot(cols)
    q = q_all[(np.arange(S) + t) % len(q_all)]
    return active.astype(np.int32), add.astype(np.int32), ids, descr, q


@pytest.mark.parametrize("S", [1, 3, 65])
def test_random_histories_in_lock_step(api, S):
    """40 steps of query, then append, with random d_active / d_add, ids advancing by 1 to 3 per stream (the cut-off window covers the last rows of every
    stream), a clear now and then, 24 rows per stream (streams fill up: ERR_CAPACITY): every output and status of every item and step equals the model, and
    at the end every stream's ids and rows do"""
    rng = np.random.default_rng(100 + S)
    cap = 24
    p = Pair(api, S, cap)
    p.canaries()
    q_all = (((3 * np.arange(DIM)[None, :] + np.arange(11)[:, None]) % 11) / 8.0).astype(np.float32)      # multiples of 1/8: one-hot rows score exactly
    next_id = [0] * S
    seen_q, seen_a = set(), set()
    for t in range(40):
        active, add, ids, descr, q = _history_step(rng, S, t, next_id, q_all)
        e = p.query(q, ids, active, min_size=2, what=("history", S, t))
        st = p.append(descr, ids, add, what=("history", S, t))
        for s in range(S):
            if st[s] == B.ADDED:
                next_id[s] = int(ids[s])
        seen_q |= set(e[4].tolist()); seen_a |= set(st)
        if t % 9 == 8:
            flags = (rng.random(S) < 0.25).astype(np.int32)
            p.clear(flags)
            for s in range(S):
                if flags[s]:
                    next_id[s] = 0
        p.check_view(("history", S, t))
    assert seen_q == {B.SCANNED, B.GATED, B.IDLE} and {B.ADDED, B.IDLE} <= seen_a
    if S == 65:
        assert B.ERR_CAPACITY in seen_a                                        # some streams fill up
    p.check_get()


# ---- 5. against the existing database ----------------------------------------------------------------------------------------------
def test_same_answers_as_three_single_databases(api):
    """S = 3: the boundary and threshold inputs loaded into three api.LoopDatabase handles as well; best id, count and score bits equal query_batch(nq = 1)"""
    import torch
    T = api.LoopDatabaseBank.row_tile()
    cap = 2 * T + 6
    cases = []
    for ps in ([T, T + 1, 1], [2 * T, cap, T - 1], [0, 1, T]):
        dbs, ids, q, cur = _boundary_inputs(T, cap, ps)
        cases.append((dbs, ids, q, cur, R.THR))
    db, q, _ = R.threshold_case()
    ids = (100 + 30 * np.arange(len(db))).astype(np.uint64)
    for thr in (R.THR, np.nextafter(R.THR, np.float32(np.inf))):
        cases.append(([db] * 3, ids, q, np.full(3, int(ids[-1]) + 25, np.uint64), thr))
    for dbs, ids, q, cur, thr in cases:
        p = Pair(api, 3, cap, mirror=False)
        got = [[], [], []]
        for s in range(3):
            p.load(s, ids, dbs[s])
            D = api.LoopDatabase(len(ids))
            rows = _t(dbs[s])
            D.append_batch(ids, rows.data_ptr(), len(ids))
            dq = _t(q[s:s + 1])
            b = torch.full((1,), SENT_I, dtype=torch.int64, device="cuda"); m = torch.full((1,), SENT_F, device="cuda"); c = torch.full((1,), SENT_I, dtype=torch.int32, device="cuda")
            D.query_batch(dq.data_ptr(), cur[s:s + 1], 1, b.data_ptr(), m.data_ptr(), c.data_ptr(), thr_low=float(thr))
            torch.cuda.synchronize()
            for k, x in enumerate((b, m, c)):
                got[k].append(x.cpu().numpy()[0])
        e = p.query(q, cur, thr=thr, what="single")
        assert np.array(got[0], np.int64).view(np.uint64).tolist() == e[0].tolist() and np.array(got[2]).tolist() == e[2].tolist()
        assert np.array(got[1], np.float32).view(np.uint32).tolist() == e[1].view(np.uint32).tolist()


# ---- 6. recorded step ---------------------------------------------------------------------------------------------------------------
def test_recorded_query_and_append_replay_against_the_model(api):
    """query + append recorded once into a StepGraph on one stream, replayed 6 times with every device input rewritten in between: each replay equals the
    model, the rows appended by earlier replays included (counts, ids and limits are read on the device)"""
    import torch
    S, cap = 3, 24
    rng = np.random.default_rng(9)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p = Pair(api, S, cap, stream=stream.cuda_stream)
        p.canaries()
        db = R.one_hot(R.spread_cols(8))
        for s in range(S):
            p.load(s, np.arange(3 + s, dtype=np.uint64) * 2, db[:3 + s])
        q_all = (((3 * np.arange(DIM)[None, :] + np.arange(11)[:, None]) % 11) / 8.0).astype(np.float32)
        dq = _t(np.zeros((S, DIM), np.float32)); dcur = _t(np.zeros(S, np.uint64)); dact = _t(np.zeros(S, np.int32)); dadd = _t(np.zeros(S, np.int32))
        ddescr = _t(np.zeros((S, DIM), np.float32)); did = _t(np.zeros(S, np.uint64))
        out = p.outputs(); ast = torch.full((S,), SENT_I, dtype=torch.int32, device="cuda")

        def body():
            p.dev.query_batch(dq.data_ptr(), dcur.data_ptr(), dact.data_ptr(), *[o.data_ptr() for o in out], thr_low=float(R.THR), min_size=3)
            p.dev.append_batch(ddescr.data_ptr(), did.data_ptr(), dadd.data_ptr(), ast.data_ptr())

        body()                                                                 # eager once, every item idle: nothing changes
        torch.cuda.synchronize()
        assert out[4].cpu().numpy().tolist() == [B.IDLE] * S and ast.cpu().numpy().tolist() == [B.IDLE] * S
        p.check_view("eager idle")
        g = api.StepGraph.record(stream.cuda_stream, [], body)
        assert g.node_count() == api.LoopDatabaseBank.launches_per_query() + 1
        next_id = [int(x[-1]) for x in p.ref.ids]
        seen = set()
        for t in range(6):
            active, add, ids, descr, q = _history_step(rng, S, t, next_id, q_all)
            if t == 0:
                active[:] = 1; add[:] = 1
            for dst, src in ((dq, q), (dcur, ids), (dact, active), (dadd, add), (ddescr, descr), (did, ids)):
                dst.copy_(_t(src))
            for o, fresh in zip(out, p.outputs()):
                o.copy_(fresh)
            ast.fill_(SENT_I)
            g.launch(stream.cuda_stream)
            torch.cuda.synchronize()
            exp = B.as_arrays(p.ref.query(q, ids, active, R.THR, 3))
            _same(p.fetch(out), exp, ("replay", t))
            seen |= set(exp[4].tolist())
            n0 = p.ref.sizes()
            want = p.ref.append(descr, ids, add)
            p.note_added(want, n0, descr, ids)
            assert ast.cpu().numpy().tolist() == want, t
            for s in range(S):
                if want[s] == B.ADDED:
                    next_id[s] = int(ids[s])
            p.check_view(("replay", t))
        assert sum(p.ref.sizes()) > 3 + 4 + 5 + 3 and B.SCANNED in seen


# ---- 7. chain ------------------------------------------------------------------------------------------------------------------------
def test_bank_outputs_feed_loop_detect(api):
    """query_batch's outputs go straight into LoopKeyFrameStore.detect_batch on the same stream, no host read in between: the scanned item with a score of 0.95 is a
    CANDIDATE at the slot of its key-frame, the gated and the idle item answer NO_LOOP"""
    import torch
    import loop_store_ref as LS
    from test_gpu_loop_store import FIVE_IDS, KEYS, Pair as StorePair
    kcap, F = 40, 16
    sp = StorePair(api, 8, kcap, F)
    kps, desc, lm = LS.random_keyframes(3, 5, kcap, F)
    assert sp.put(FIVE_IDS, kps, desc, [5, 9, kcap - 1, kcap, 7], None, lm, [3, 4, F, 2, 1]) == 0
    S, cap = 3, 12
    p = Pair(api, S, cap)
    ids = np.array(FIVE_IDS, np.uint64)                                        # stream 0's database holds the store's key-frames
    db = R.one_hot(R.spread_cols(5))
    p.load(0, ids, db); p.load(1, ids[:2], db[:2]); p.load(2, ids, db)
    q = np.zeros((S, DIM), np.float32)
    q[:, R.spread_cols(5)[2]] = 0.95; q[:, R.spread_cols(5)[0]] = 0.5
    cur = np.full(S, 2 ** 41, np.uint64)
    dq, dc, da = _t(q), _t(cur), _t(np.array([1, 1, 0], np.int32))
    out = p.outputs()
    sout = sp.outputs(S)
    p.dev.query_batch(dq.data_ptr(), dc.data_ptr(), da.data_ptr(), *[o.data_ptr() for o in out], thr_low=float(R.THR), min_size=2)
    sp.launch(out[:3], sout)
    torch.cuda.synchronize()
    got = p.fetch(out)
    _same(got, B.as_arrays(p.ref.query(q, cur, [1, 1, 0], R.THR, 2)), "chain")
    assert got[4].tolist() == [B.SCANNED, B.GATED, B.IDLE] and got[0][0] == FIVE_IDS[2] and got[1][0] == np.float32(0.95) and got[3][0] == 2
    want = sp.ref.detect(got[0], got[1], got[2], np.float32(0.94), 3, LS.sentinel_outputs(S, kcap, F))
    for k in KEYS:
        assert sout[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert want["status"].tolist() == [0, 1, 1] and want["slot"].tolist() == [2, -1, -1] and want["n_loop"].tolist() == [kcap - 1, 0, 0]


# ---- 8. accuracy on real-valued data ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "relu", "wide"])
def test_scores_are_as_accurate_as_the_reference_loop(api, oracle, kind):
    """e = |score - f64| / (u * A), u = 2^-24, A = |row| . |query|, for each of 300 x 40 pairs: max e(bank) <= max e(oracle's own f32 loop, orc_lcd_score)
    on the same pairs, no extra factor — a lane adds 16 to 20 products in one chain and the 64 lane sums meet in a six-level tree, the sequential loop's
    chain is 1063 additions long.

    600 streams of 40 slots: row r sits alone among zero rows of stream r (the slot wanders over the waves of both tiles), the row times 2^8 likewise in stream
    300 + r; one call per query covers all rows.  The sign of each stream's query is chosen so that the pair's score is positive (negation is exact in every
    step), and the queries of the upper 300 streams are scaled by 2^-5: their scores must be the lower ones' bits times 2^3.

    Measured on an MI355X (max e: bank / oracle loop): gauss 0.34 / 4.10, relu 2.23 / 10.33, wide 2.59 / 20.19."""
    from test_gpu_lcddb_scan import _accuracy_set
    db, q = _accuracy_set(kind)
    S64, A = R.scores64(db, q)
    assert (A > 0).all() and (S64 != 0).all()
    sign = np.where(S64 < 0, -1.0, 1.0).astype(np.float32)
    nr, nq, cap = len(db), len(q), 40
    p = Pair(api, 2 * nr, cap, mirror=False)
    ids = (100 + 30 * np.arange(cap)).astype(np.uint64)
    slot = (np.arange(nr) * 7) % cap
    block = np.zeros((cap, DIM), np.float32)
    for r in range(nr):
        for s, row in ((r, db[r]), (nr + r, db[r] * np.float32(256))):
            block[:] = 0; block[slot[r]] = row
            p.dev.load(s, ids, block)
    cur = _t(np.full(2 * nr, int(ids[-1]) + 25, np.uint64))
    got = np.zeros((nr, nq), np.float32); scaled = np.zeros((nr, nq), np.float32)
    out = p.outputs()
    for i in range(nq):
        qs = q[i][None, :] * sign[:, i][:, None]
        dq = _t(np.concatenate([qs, qs * np.float32(2.0 ** -5)]))
        p.dev.query_batch(dq.data_ptr(), cur.data_ptr(), 0, *[o.data_ptr() for o in out], thr_low=0.0)
        p.torch.cuda.synchronize()
        f = p.fetch(out)
        assert (f[4] == B.SCANNED).all() and (f[3] == np.concatenate([slot, slot])).all() and (f[2] == 1).all(), (kind, i)
        got[:, i] = f[1][:nr]; scaled[:, i] = f[1][nr:]
    ref_abs = np.abs(S64)
    e_or = np.zeros_like(S64)
    for r in range(nr):
        for i in range(nq):
            e_or[r, i] = abs(float(oracle.lcd_score(q[i] * sign[r, i], db[r])) - ref_abs[r, i])
    e_or = e_or / (R.U * A)
    e_bank = float((np.abs(got.astype(np.float64) - ref_abs) / (R.U * A)).max())
    line = f"{kind}: max e bank {e_bank:.2f}, oracle loop {e_or.max():.2f}"
    print(line)
    assert np.array_equal((got * np.float32(8)).view(np.uint32), scaled.view(np.uint32)), (kind, "scaling by 2^8 and 2^-5 is not exact")
    assert e_bank <= e_or.max(), line


# ---- 9. facade ------------------------------------------------------------------------------------------------------------------------
def test_cpp_facade_bank(api, tmp_path):
    """myslam::LoopDatabaseBank (host/myslam_hip.hpp) in a compiled host program: tests/cpp/lcd_bank_test.cpp against the literal loop of DetectLoop"""
    from conftest import PKG_DIR, ROOT
    exe = str(tmp_path / "lcd_bank_test")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "lcd_bank_test.cpp"), "-o", exe,
           "-L" + PKG_DIR, "-lmyslam_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "LCD BANK TEST OK" in r.stdout, r.stdout + r.stderr
