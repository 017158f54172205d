"""CPU: pins tests/lcddb_scan_ref.py — the restatement the GPU tests of the loop-database scan hold the kernels to — against the oracle's scan and the
library's host merges, and asserts what every constructed input of tests/test_gpu_lcddb_scan.py is made of."""
import numpy as np
import pytest

import lcddb_scan_ref as R

M64 = R.M64


def _oracle_scores(oracle, db, q):
    return np.array([[oracle.lcd_score(q[i], db[r]) for i in range(len(q))] for r in range(len(db))], np.float32)


def _id_sets():
    top = [M64 - k for k in (40, 25, 19, 18, 7, 2, 1)]
    return {"spaced": [7 + 3 * r for r in range(60)],
            "from_zero": list(range(0, 60)),
            "high": [M64 - 500 + 7 * r for r in range(60)],
            "wrapping_tail": [30 + 11 * r for r in range(53)] + top,
            "only_tail": top,
            "single": [19]}


def test_scan_equals_the_oracle_scan(oracle, synth):
    """scan() on the oracle's own f32 scores gives the oracle's answer for every cur: 0, 18, 19, 20, below / inside / above the id range, ids at 2^64 - k,
    an empty prefix"""
    rng = np.random.default_rng(1)
    base = synth.lcd_database(60, seed=31)
    base[::2] *= -1                                                       # negative scores exist
    base[17] = base[5]                                                    # and exact ties
    qs = np.stack([base[5], base[40] * 0.9 + base[3] * 0.1, -base[8]]).astype(np.float32)
    empty = 0
    for name, ids in _id_sets().items():
        ids = np.array(ids, dtype=np.uint64); n = len(ids)
        db = np.ascontiguousarray(base[:n])
        S = _oracle_scores(oracle, db, qs)
        curs = [0, 18, 19, 20, 21, 38, 39, 40, M64 - 1, M64 - 2, M64 - 19, M64 - 20, M64 - 21]
        for i in ids[[0, n // 2, n - 1]]:
            curs += [(int(i) + d) % M64 for d in (-1, 0, 1, 19, 20)]
        curs += [int(c) for c in rng.integers(0, 400, 10)]
        for cur in curs:
            for thr in (R.THR, np.float32(0.1), np.float32(-0.2)):
                for i in range(len(qs)):
                    got = R.scan(S[:, i], ids, cur, thr)
                    ref = oracle.lcddb_query(db, ids, qs[i], cur, thr_low=float(thr))
                    assert (got[0], float(got[1]), got[2]) == ref, (name, cur, float(thr), i, got, ref)
            empty += R.in_window(cur, ids[0])
            # the other statements of the same rule agree with the loop
            rb, rm, rc = R.shard_record(S[:, 0], ids, cur)
            assert (rb, rm, rc & 0x7fffffff) == R.scan(S[:, 0], ids, cur) and (rc < 0) == any(R.in_window(cur, i) for i in ids)
    assert empty > 10


def test_nan_never_wins_and_is_never_counted():
    ids = np.arange(5, dtype=np.uint64)
    s = np.array([0.5, np.nan, 0.95, np.nan, 0.93], np.float32)
    assert R.scan(s, ids, 100) == (2, np.float32(0.95), 2)
    assert R.scan(np.full(5, np.nan, np.float32), ids, 100) == (0, np.float32(0), 0)
    assert R.scan(s, ids, 100, np.float32(-1)) == (2, np.float32(0.95), 3)


def _records(S, parts, cur, fn):
    return [[fn(S[rows, i], ids, cur[i]) for i in range(len(cur))] for rows, ids in parts]


def test_merges_equal_one_scan_and_the_library_host_merges(pkg):
    """id-range shards + merge() and interleaved shards + merge_owned() both give scan() of the whole map; the library's host entry points (no device
    needed) give the same arrays from the same records"""
    import ctypes
    api = pkg.api
    ctypes.CDLL(pkg.build_library())
    db, ids, q, cur = R.whole_map_case()
    S = R.exact32(R.scores64(db, q)[0])
    n = len(ids)
    whole = R.scan_many(S, ids, cur)
    assert len(set(whole[0].tolist())) > 10 and (whole[2] > 0).any()
    for cuts in ([0, 128, 161, n], [0, 1, 2, n], [0, n]):
        parts = [(np.arange(a, b), ids[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        rec = _records(S, parts, cur, R.shard_record)
        got = R.merge(rec)
        assert all(np.array_equal(g, w) for g, w in zip(got, whole)), cuts
        lib = api.lcd_merge_candidates(np.array(rec, dtype=api.CAND_DTYPE))
        assert all(np.array_equal(g, w) for g, w in zip(lib, got)), cuts
    for ns in (1, 2, 3, 8):
        for order in (1, -1):
            parts = [(np.arange(s, n, ns), ids[s::ns]) for s in range(ns)][::order]
            rec = _records(S, parts, cur, R.owned_record)
            got = R.merge_owned(rec)
            assert all(np.array_equal(g, w) for g, w in zip(got, whole)), (ns, order)
            lib = api.lcd_merge_owned_candidates(np.array(rec, dtype=api.OWNED_DTYPE))
            assert all(np.array_equal(g, w) for g, w in zip(lib, got)), (ns, order)


def test_owned_merge_keeps_the_prefix_id_on_equal_scores():
    rec = [[(7, np.float32(0.5), 1, 90, np.float32(0.5), 2)], [(5, np.float32(0.5), 0, 80, np.float32(0.75), 0)]]
    assert [x[0] for x in R.merge_owned(rec)] == [80, np.float32(0.75), 3]
    rec[1][0] = (5, np.float32(0.5), 0, 80, np.float32(0.5), 0)
    assert [x[0] for x in R.merge_owned(rec)] == [5, np.float32(0.5), 3]
    rec[0][0] = (7, np.float32(0.5), 1 + R.BREAK, 90, np.float32(0.9), 2)
    assert [x[0] for x in R.merge_owned(rec)] == [5, np.float32(0.5), 1]


def test_bf16_split3():
    x = np.array([1.0, R.A3, R.A2, -R.A3, 0.92, 3.0e-5, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0], np.float32)
    h, m, l = R.bf16_split3(x)
    assert np.array_equal((l.astype(np.float64) + m) + h, x.astype(np.float64))
    for p in (h, m, l):
        assert (p.view(np.uint32) & 0xffff == 0).all()
    assert h[6] == 1.0 and h[7] == np.float32(1 + 2.0 ** -6)              # ties go to the even bf16
    assert (h[1], m[1], l[1]) == (1.0, 2.0 ** -9, 2.0 ** -17) and (h[2], m[2], l[2]) == (1.0, 2.0 ** -9, 0.0)


# ---- what the constructed inputs of the GPU tests are made of ----------------------------------------------------------------
def test_one_hot_inputs():
    for db, q in (R.one_hot_rows_case(), R.one_hot_queries_case()):
        assert R.one_term_ok(db, q)
        S = R.exact32(R.scores64(db, q)[0])
        oh, other = (db, q) if (db != 0).sum(axis=1).max() == 1 else (q, db)
        assert sorted(set(np.nonzero(oh)[1].tolist())) == sorted(R.ONE_HOT_K) and set(oh[oh != 0].tolist()) == {1.0}
        mag = np.abs(other[other != 0])
        assert mag.min() < 2.0 ** -18 and mag.max() > 2.0 ** 18 and (other < 0).any() and (np.abs(other[:, list(R.ONE_HOT_K)]) >= 1).all()
        assert (S > 0).any() and (S < 0).any()
    db, q = R.one_hot_rows_case()
    best = R.scan_many(R.exact32(R.scores64(db, q)[0]), np.arange(len(db)), np.full(len(q), 10 ** 6))[0]
    assert best.tolist() == list(range(len(R.ONE_HOT_K)))                 # every column of the sweep is some query's answer


def test_product_inputs_and_every_product_matters():
    seen = set()
    for name, (row, q, n, g, need) in R.product_cases().items():
        assert R.grid_ok(row[None], q, g) and n * float(np.abs(row).max() * np.abs(q).max()) < 2.0 ** (24 - g)
        cols = np.nonzero(row)[0]
        assert len(cols) == n and (cols % 16 < 8).any() and (cols % 16 >= 8).any() and len(set((cols // 16).tolist())) > 20 and (cols >= 1056).sum() == 8
        full = float(R.scores64(row[None], q)[0][0, 0])
        assert full == float(np.float32(full)) == R.six_product_value(row, q)          # the three products the kernel drops are zero here
        for p in R.PRODUCTS:
            assert (R.six_product_value(row, q, leave_out=p) != full) == (p in need), (name, p)
        seen |= set(need)
    assert seen == set(R.PRODUCTS)
    h, m, l = R.bf16_split3(np.array([R.A3, R.A2], np.float32))
    assert (h[0], m[0], l[0]) == (1.0, 2.0 ** -9, 2.0 ** -17) and (h[1], m[1], l[1]) == (1.0, 2.0 ** -9, 0.0)


def test_threshold_inputs():
    db, q, V = R.threshold_case()
    assert R.one_term_ok(db, q) and np.array_equal(R.exact32(R.scores64(db, q)[0]), V)
    up, dn = np.nextafter(R.THR, np.float32(np.inf)), np.nextafter(R.THR, np.float32(-np.inf))
    assert dn < R.THR < up and up.view(np.uint32) - dn.view(np.uint32) == 2
    assert (V[:, 0] == up).sum() == 1 and (V[:, 0] == R.THR).sum() == 2 and (V[:, 1] <= 0).all() and (V[:, 1] < 0).any()
    assert np.signbit(q[q == 0]).any()                                    # a -0.0 is among the inputs


@pytest.mark.parametrize("n,far", [(2049, (0, 2048)), (2049, (33, 2048)), (8193, (5, 8192)), (8193, (130, 8192))])
def test_tie_inputs(n, far):
    groups = R.tie_groups(n, *far)
    db, q = R.tie_case(n, groups)
    assert R.grid_ok(db[:300], q, 2) and R.grid_ok(db[[r for g in groups for r in g]], q, 2)
    S = R.exact32(R.scores64(db, q)[0])
    for g, rows in enumerate(groups):
        assert all(np.array_equal(db[r].view(np.uint32), q[g].view(np.uint32)) for r in rows)
        assert sorted(np.nonzero(S[:, g] == S[:, g].max())[0].tolist()) == sorted(rows) and S[:, g].max() == 1.25
    for (a, b), off in zip(groups, R.TIE_OFFSETS):
        assert b - a == off and a % 256 == 1
    rows_per = 32 if n == 2049 else 128
    lo, hi = far
    assert hi // rows_per == 64 and lo // rows_per in (0, 1) and (n + rows_per - 1) // rows_per == 65


def test_limit_inputs():
    for n in (1, 31, 32, 33, 127, 128, 129, 257):
        lim = [p for p in R.LIMITS if p <= n] + [n + 1]
        db, ids, q, cur = R.limit_case(n, lim)
        assert R.one_term_ok(db, q)
        S = R.exact32(R.scores64(db, q)[0])
        best, mx, cnt = R.scan_many(S, ids, cur)
        for i, p in enumerate(lim):
            seen = sum(1 for r in range(n) if not any(R.in_window(cur[i], ids[k]) for k in range(r + 1)))
            assert seen == min(p, n)
            if p < n:
                assert S[p, i] == S[:, i].max() == 4
            if p <= n:
                assert (best[i], mx[i]) == ((ids[p - 1], 2) if p >= 1 else (0, 0))
            else:
                assert mx[i] == S[:, i].max() <= 1


def test_owned_inputs():
    db, ids, q, cur = R.owned_start_case()
    assert R.one_term_ok(db, q)
    rng = [R.owned_ranges(ids, c) for c in cur]
    assert {r[2] for r in rng if not r[1]} >= set(R.LIMITS) and {r[0] for r in rng} >= set(R.LIMITS)
    assert {r[2] for r in rng if r[1]} >= {t + 1 for t in R.LIMITS} and any(r[2] == r[3] for r in rng) and any(r[2] < r[3] for r in rng)
    ends = set()
    for t0, small in ((0, ()), (31, (3, 10)), (64, ()), (127, ())):
        db, ids, q, cur = R.owned_wrap_case(t0, small)
        assert R.one_term_ok(db, q) and ids[-1] == M64 - 1 and (np.diff(ids.astype(object)) > 0).all()
        rng = [R.owned_ranges(ids, c) for c in cur]
        ends |= {r[3] for r in rng[:19]}
        assert all(r[0] == 0 for r in rng[:19]) and [r[3] for r in rng[:19]] == [t0 + c for c in range(19)]
        if small:
            assert any(r[1] and r[2] > 0 for r in rng[:19]) and any(not r[1] for r in rng[:19])
    assert ends >= set(R.LIMITS)
    db, ids, q, cur = R.whole_map_case()
    assert R.one_term_ok(db, q)
