"""Pins tests/lcd_bank_ref.py, the plain-Python model of the loop database bank: the empty answers of gated and idle items, AddToDatabase's refusals,
the wrapping cut-off window against lcddb_scan_ref.scan, and the sizes of a random history against a count the test keeps itself.  No device."""
import numpy as np

import lcd_bank_ref as B
import lcddb_scan_ref as R


def _rows(n, seed=0):
    return R.one_hot((np.arange(n) * 37 + 5 + seed) % R.DIM)


def test_gated_and_idle_items_give_the_empty_answer():
    bank = B.Bank(4, 10)
    db = _rows(6)
    bank.load(0, range(100, 106), db)
    bank.load(1, range(100, 103), db[:3])
    bank.load(3, range(100, 106), db)
    q = np.stack([db[2] * 0.95] * 4).astype(np.float32)
    out = bank.query(q, [1000] * 4, active=[1, 1, 1, 0], min_size=3)
    assert out[0][4] == B.SCANNED and out[0][:4] == (102, np.float32(0.95), 1, 2)
    for s, st in ((1, B.GATED), (2, B.GATED), (3, B.IDLE)):            # n == min_size, n == 0, not active
        assert out[s] == (0, 0.0, 0, -1, st) and isinstance(out[s][1], np.float32)
    assert bank.query(q, [1000] * 4, min_size=2)[1][4] == B.SCANNED     # the gate is strict: n > min_size scans
    assert bank.query(q, [1000] * 4, min_size=6)[0] == (0, 0.0, 0, -1, B.GATED)
    z = bank.query(np.zeros_like(q), [1000] * 4)[0]                      # a scan that finds nothing above 0 names no row
    assert z == (0, 0.0, 0, -1, B.SCANNED)
    a = B.as_arrays(out)
    assert [x.dtype for x in a] == [np.uint64, np.float32, np.int32, np.int32, np.int32] and a[4].tolist() == [B.SCANNED, B.GATED, B.GATED, B.IDLE]


def test_append_refuses_equal_lower_and_full_and_changes_nothing():
    bank = B.Bank(5, 3)
    db = _rows(3)
    bank.load(0, [5, 7], db[:2]); bank.load(1, [5, 7], db[:2]); bank.load(2, [5, 7, 9], db); bank.load(4, [5], db[:1])
    before = ([list(x) for x in bank.ids], [[r.copy() for r in x] for x in bank.rows])
    new = _rows(5, seed=400)
    st = bank.append(new, [7, 6, 100, 0, 100], add=[1, 1, 1, 1, 0])
    assert st == [B.ERR_INVALID, B.ERR_INVALID, B.ERR_CAPACITY, B.ADDED, B.IDLE]
    for s in (0, 1, 2, 4):
        assert bank.ids[s] == before[0][s] and all(np.array_equal(a, b) for a, b in zip(bank.rows[s], before[1][s]))
    assert bank.ids[3] == [0] and np.array_equal(bank.rows[3][0], new[3]) and bank.sizes() == [2, 2, 3, 1, 1]
    assert bank.append(new, [8, 8, 8, 8, 8]) == [B.ADDED, B.ADDED, B.ERR_CAPACITY, B.ADDED, B.ADDED]      # add=None selects every stream
    assert bank.append(new, [9] * 5) == [B.ERR_CAPACITY, B.ERR_CAPACITY, B.ERR_CAPACITY, B.ADDED, B.ADDED]      # a full stream says so before it looks at the id
    bank.clear([0, 0, 1, 0, 0])
    assert bank.sizes() == [3, 3, 0, 3, 3] and bank.append(new, [0] * 5, add=[0, 0, 1, 0, 0])[2] == B.ADDED


def test_wrapping_window_equals_the_scan():
    """the streams of one bank hold owned_wrap_case's ids (the last 19 at 2^64 - 19 ..): every query, cur < 19 among them, gives what scan() gives"""
    for t0, small in ((0, ()), (31, (3, 10)), (64, ())):
        db, ids, q, cur = R.owned_wrap_case(t0, small)
        nq = len(q)
        bank = B.Bank(nq, len(ids))
        for s in range(nq):
            bank.load(s, ids, db)
        S = R.exact32(R.scores64(db, q)[0])
        out = bank.query(q, cur)
        for s in range(nq):
            best, mx, cnt = R.scan(S[:, s], ids, cur[s])
            assert out[s][:3] == (best, mx, cnt) and out[s][4] == B.SCANNED
            assert out[s][3] == (ids.tolist().index(best) if mx > 0 else -1)
        for c in range(19):
            if not small:
                assert out[c][3] == t0 + c - 1 and out[c][1] == (2 if t0 + c else 0)      # the row in front of the wrapped window


def test_random_history_sizes():
    rng = np.random.default_rng(5)
    S, cap = 7, 6
    bank = B.Bank(S, cap)
    count = [0] * S; last = [-1] * S
    seen = set()
    for step in range(60):
        add = rng.integers(0, 2, S)
        ids = [max(0, last[s] + int(rng.integers(0, 3))) for s in range(S)]    # now and then an id that does not ascend
        st = bank.append(_rows(S, seed=step), ids, add)
        for s in range(S):
            if add[s] and count[s] < cap and ids[s] > last[s]:
                count[s] += 1; last[s] = ids[s]
        seen |= set(st)
        if step % 17 == 16:
            flags = rng.integers(0, 2, S)
            bank.clear(flags)
            for s in range(S):
                if flags[s]:
                    count[s] = 0; last[s] = -1
        assert bank.sizes() == count
    assert seen == {B.ADDED, B.IDLE, B.ERR_INVALID, B.ERR_CAPACITY}
