"""The loop-database scan (csrc/lcddb.hip) restated in plain numpy and Python loops, with f64 scores.

The scan rule is LoopClosing::DetectLoop (reference src/loopclosing.cpp:124-161) as the oracle's orc_lcddb_query states it: ids ascend, the walk
ends at the first id with (cur - id) mod 2^64 < 20, the maximum starts at 0 with best id 0, '>' is strict for the maximum and for the count, and
a NaN score never wins and is never counted.  The shard records and the two merges follow the comments above k_db_pack_candidates,
k_db_pack_owned and scan_ranges.  Nothing here looks at the device; tests/test_lcddb_scan_ref.py pins it against the oracle and the library's
host merges, tests/test_gpu_lcddb_scan.py holds the kernels to it.

Also here: the builders of the constructed inputs those tests feed to the kernels, so that the CPU file can assert what each one is made of."""
import numpy as np

DIM = 1064
U = 2.0 ** -24                     # unit roundoff of f32: errors are judged in units of U * A, A = |db| @ |q|.T
M64 = 1 << 64
THR = np.float32(0.92)             # LoopClosing's thr_low
BREAK = -(1 << 31)                 # bit 31 of an int32 count: this shard's scan hit the break


def scores64(db, q):
    """(S, A): the f64 scores db @ q.T [rows, queries] and their magnitudes |db| @ |q|.T"""
    d = np.asarray(db, np.float32).astype(np.float64); qq = np.atleast_2d(np.asarray(q, np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return d @ qq.T, np.abs(d) @ np.abs(qq).T


def exact32(S):
    """f64 scores that ARE f32 numbers, as f32 (the constructed inputs: no rounding anywhere, so no tolerance)"""
    S32 = S.astype(np.float32)
    ok = (S32.astype(np.float64) == S) | np.isnan(S)
    assert ok.all(), "constructed scores must be exactly representable in f32"
    return S32


def in_window(cur, i):
    return (int(cur) - int(i)) % M64 < 20


def _list(a):
    return a.tolist() if isinstance(a, np.ndarray) else [x.item() if isinstance(x, np.generic) else x for x in a]


def _walk(scores, ids, rows, thr_low):
    """the body of the scan over the given rows: (best_id, max_score, cnt), starting from (0, 0.0, 0)"""
    thr = float(np.float32(thr_low))
    scores = _list(np.asarray(scores, np.float32)); ids = _list(ids)
    best, mx, cnt = 0, 0.0, 0
    for r in rows:
        s = scores[r]
        if s > mx:                 # strict: the first (lowest-id) maximum stays; NaN compares false
            mx = s; best = ids[r]
        if s > thr:
            cnt += 1
    return best, mx, cnt


def scan(scores_col, ids, cur, thr_low=THR):
    """the literal loop of loopclosing.cpp:124-161 over one column of f32 scores -> (best_id, max_score, cnt)"""
    best, mx, cnt = 0, 0.0, 0
    thr = float(np.float32(thr_low))
    scores = _list(np.asarray(scores_col, np.float32)); ids = _list(ids); cur = int(cur)
    for r in range(len(ids)):
        if (cur - ids[r]) % M64 < 20:
            break
        s = scores[r]
        if s > mx:
            mx = s; best = ids[r]
        if s > thr:
            cnt += 1
    return best, np.float32(mx), cnt


def scan_many(S32, ids, cur, thr_low=THR):
    """scan() of every column -> arrays (best_id u64, max_score f32, cnt i32)"""
    nq = S32.shape[1]
    best = np.zeros(nq, np.uint64); mx = np.zeros(nq, np.float32); cnt = np.zeros(nq, np.int32)
    for i in range(nq):
        best[i], mx[i], cnt[i] = scan(S32[:, i], ids, cur[i], thr_low)
    return best, mx, cnt


def shard_record(scores_col, ids, cur, thr_low=THR):
    """What a shard that owns an ascending id RANGE reports (k_db_pack_candidates): its own scan, bit 31 of cnt = the scan hit the break."""
    ids = _list(ids); cur = int(cur)
    broke = False
    rows = []
    for r in range(len(ids)):
        if (cur - ids[r]) % M64 < 20:
            broke = True
            break
        rows.append(r)
    best, mx, cnt = _walk(scores_col, ids, rows, thr_low)
    return best, np.float32(mx), cnt + (BREAK if broke else 0)


def owned_ranges(ids, cur):
    """(p, broke, sb, se) of a shard whose ids interleave with other shards' (scan_ranges): rows [0, p) lie below the cut-off window
    W = {id : (cur - id) mod 2^64 < 20}; broke = the shard holds an id of W that is <= cur; rows [sb, se) are the ids above cur that lie below the part of
    W that wraps around 2^64 (cur < 19: ids >= 2^64 - (19 - cur))."""
    cur = int(cur); ids = _list(ids)
    lo = cur - 19 if cur >= 19 else 0
    p = sum(1 for i in ids if i < lo)
    broke = any(lo <= i <= cur for i in ids)
    sb = sum(1 for i in ids if i <= cur)
    se = sum(1 for i in ids if not (i > cur and (cur - i) % M64 < 20))          # ids ascend: the wrapped part of W is a tail of the shard
    return p, broke, sb, max(se, sb)


def owned_record(scores_col, ids, cur, thr_low=THR):
    """(pre_best_id, pre_max_score, pre_cnt | break bit, suf_best_id, suf_max_score, suf_cnt) of one shard (k_db_pack_owned)"""
    p, broke, sb, se = owned_ranges(ids, cur)
    pb, pm, pc = _walk(scores_col, ids, range(0, p), thr_low)
    sbest, sm, sc = _walk(scores_col, ids, range(sb, se), thr_low)
    return pb, np.float32(pm), pc + (BREAK if broke else 0), sbest, np.float32(sm), sc


def merge(records):
    """records[shard][query] = (best_id, max_score, cnt) of shards in ascending id-range order -> arrays of the ONE scan they make up"""
    ns, nq = len(records), len(records[0])
    best = np.zeros(nq, np.uint64); mx = np.zeros(nq, np.float32); cnt = np.zeros(nq, np.int32)
    for i in range(nq):
        b, m, c = 0, 0.0, 0
        for s in range(ns):
            rb, rm, rc = records[s][i]
            if float(rm) > m:
                m = float(rm); b = int(rb)
            c += int(rc) & 0x7fffffff
            if int(rc) < 0:
                break
        best[i], mx[i], cnt[i] = b, m, c
    return best, mx, cnt


def merge_owned(records):
    """records[shard][query] = owned_record(...) of shards in ANY order -> arrays of the one scan of the whole map"""
    ns, nq = len(records), len(records[0])
    best = np.zeros(nq, np.uint64); mx = np.zeros(nq, np.float32); cnt = np.zeros(nq, np.int32)
    for i in range(nq):
        b, m, c, broke = 0, 0.0, 0, False
        for s in range(ns):                                   # everything below the window: highest score, lowest id among equals
            pb, pm, pc = records[s][i][:3]
            if float(pm) > m or (float(pm) == m and m > 0 and int(pb) < b):
                m = float(pm); b = int(pb)
            c += int(pc) & 0x7fffffff
            broke = broke or int(pc) < 0
        if not broke:                                         # nothing inside the window: the scan goes on above cur
            sm, sbest = 0.0, 0
            for s in range(ns):
                xb, xm, xc = records[s][i][3:]
                if float(xm) > sm or (float(xm) == sm and sm > 0 and int(xb) < sbest):
                    sm = float(xm); sbest = int(xb)
                c += int(xc)
            if sm > m:                                        # strict: an equal score further up the map does not replace the earlier one
                m = sm; b = sbest
        best[i], mx[i], cnt[i] = b, m, c
    return best, mx, cnt


def bf16_rne(x):
    """f32 -> the nearest bf16 (ties to even), returned as f32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_split3(x):
    """(h, m, l): x split into three bf16 pieces by round-to-nearest-even, each as f32 (bf16_split3 of csrc/wave_ops.h)"""
    x = np.asarray(x, np.float32)
    h = bf16_rne(x); r = (x - h).astype(np.float32)
    m = bf16_rne(r); q = (r - m).astype(np.float32)
    return h, m, bf16_rne(q)


# ---- constructed inputs ------------------------------------------------------------------------------------------------------
ONE_HOT_K = (0, 1, 7, 8, 15, 16, 63, 64, 1023, 1024, 1039, 1055, 1056, 1063)      # GEMV lane / tail boundaries, GEMM k halves, the half-empty last stage


def one_hot(cols, value=1.0):
    a = np.zeros((len(cols), DIM), np.float32)
    a[np.arange(len(cols)), np.asarray(cols)] = value
    return a


def spread_cols(n):
    """n distinct columns that wander over every k position (37 and 1064 are coprime)"""
    assert n <= DIM
    return (np.arange(n) * 37 + 5) % DIM


def mixed_vector(seed, keep_cols):
    """one vector of mixed magnitudes 2^-20 .. 2^20 and signs, 24-bit significands; the entries at keep_cols are at least 1 in magnitude"""
    rng = np.random.default_rng(seed)
    v = (1.0 + rng.integers(0, 1 << 23, DIM) / float(1 << 23)) * np.exp2(rng.integers(-20, 21, DIM)) * rng.choice([-1.0, 1.0], DIM)
    kc = np.asarray(keep_cols)
    v[kc] = (1.0 + rng.integers(0, 1 << 23, len(kc)) / float(1 << 23)) * np.exp2(rng.integers(0, 21, len(kc))) * rng.choice([-1.0, 1.0], len(kc))
    v = v.astype(np.float32)
    assert (np.abs(v[kc]) >= 1).all()
    return v


def product_positions(n):
    """n columns in both k halves of a stage (k mod 16 below and from 8), in many stages, and the 8 columns of the tail stage 1056 .. 1063"""
    body = (np.arange(n - 8) * 17 + 3) % 1056
    cols = np.concatenate([body, np.arange(1056, 1064)])
    assert len(set(cols.tolist())) == n
    return cols


A3 = np.float32(1 + 2.0 ** -9 + 2.0 ** -17)      # pieces 1, 2^-9, 2^-17
A2 = np.float32(1 + 2.0 ** -9)                   # pieces 1, 2^-9, 0
PRODUCTS = ("hh", "hm", "mh", "hl", "lh", "mm")  # (piece of the row, piece of the query) the kernel accumulates


def product_cases():
    """name -> (row, query, N, g, products that carry the score): row . query = N * a * q is exact on the 2^-g grid, so any f32 order is exact"""
    out = {}
    for name, a, q, n, g, need in (("row_hml", A3, np.float32(1), 64, 17, ("hh", "mh", "lh")),
                                   ("query_hml", np.float32(1), A3, 64, 17, ("hh", "hm", "hl")),
                                   ("mm", A2, A2, 32, 18, ("hh", "hm", "mh", "mm"))):
        cols = product_positions(n)
        row = np.zeros(DIM, np.float32); qv = np.zeros(DIM, np.float32)
        row[cols] = a; qv[cols] = q
        out[name] = (row, qv, n, g, need)
    return out


def six_product_value(row, q, leave_out=None):
    """the score as the sum of the kernel's six piece products in f64, optionally without one of them"""
    pa = dict(zip("hml", [p.astype(np.float64) for p in bf16_split3(row)]))
    pq = dict(zip("hml", [p.astype(np.float64) for p in bf16_split3(q)]))
    return sum(float(pa[x[0]] @ pq[x[1]]) for x in PRODUCTS if x != leave_out)


def grid_ok(db, q, g):
    """every term a_k * q_k is a multiple of 2^-g and (number of nonzero terms) * max|term| < 2^(24-g): every partial sum in every order is an f32 number"""
    d = np.asarray(db, np.float64)[:, None, :] * np.atleast_2d(np.asarray(q, np.float64))[None, :, :]
    t = d * 2.0 ** g
    n = (d != 0).sum(axis=2).max()
    return bool((t == np.round(t)).all()) and float(n * np.abs(d).max()) < 2.0 ** (24 - g)


def pairs_exact(db, q):
    """grid_ok with every (row, query) pair on its own grid: g = the finest bit any of the pair's terms uses"""
    d = np.asarray(db, np.float64)[:, None, :] * np.atleast_2d(np.asarray(q, np.float64))[None, :, :]
    g = np.zeros(d.shape[:2])
    for k in range(1, 60):
        t = d * 2.0 ** (k - 1)
        g = np.where((t != np.round(t)).any(axis=2), k, g)
    n = (d != 0).sum(axis=2)
    return bool((n * np.abs(d).max(axis=2) < 2.0 ** (24 - g)).all())


def one_term_ok(db, q):
    """every (row, query) pair has at most ONE nonzero term, and the three pieces of every entry sum back to it in the kernel's order (l + m) + h:
    the score is that term, exactly, on both kernels"""
    nz = (np.asarray(db)[:, None, :] != 0) & (np.atleast_2d(q)[None, :, :] != 0)
    ok = int(nz.sum(axis=2).max()) <= 1
    for x in (np.asarray(db, np.float32), np.atleast_2d(np.asarray(q, np.float32))):
        h, m, l = bf16_split3(x)
        back = ((l + m).astype(np.float32) + h).astype(np.float32)
        ok = ok and bool(((back == x) | np.isnan(x)).all())
        tiny = np.abs(np.stack([h, m, l])[np.stack([h, m, l]) != 0])
        ok = ok and (tiny.size == 0 or float(np.nanmin(tiny)) >= 2.0 ** -126)      # no piece is subnormal
    return ok


def one_hot_rows_case():
    """42 one-hot rows that sweep ONE_HOT_K three times (two GEMV blocks); query j is a mixed vector whose largest positive entry sits at
    column ONE_HOT_K[j], so that every column is some query's answer"""
    K = list(ONE_HOT_K)
    db = one_hot([K[r % len(K)] for r in range(3 * len(K))])
    q = np.stack([mixed_vector(100 + j, K) for j in range(len(K))])
    for j, k in enumerate(K):
        q[j, k] = np.float32(2.0 ** 21 * (1 + (2 * j + 1) / 64.0 + 2.0 ** -23))
    return db, q


def one_hot_queries_case():
    """the roles swapped: 42 mixed rows, one one-hot query per column of ONE_HOT_K"""
    K = list(ONE_HOT_K)
    db = np.stack([mixed_vector(200 + r, K) for r in range(3 * len(K))])
    return db, one_hot(K)


def threshold_case():
    """one-hot rows; query i gives row r the score V[i][r] (0 beyond the list).  Query 0: the threshold, its two neighbours, zeros and negatives; query 1:
    nothing above 0; query 2: as query 0 in another order, neighbours first"""
    up, dn = np.nextafter(THR, np.float32(np.inf)), np.nextafter(THR, np.float32(-np.inf))
    V = [[0.5, THR, dn, 0.0, -0.0, -1.5, up, -THR, dn, THR, 0.25],
         [0.0, -0.0, -1.5, -THR, -0.25, -0.0, 0.0, -2.0 ** -20, -3.0, 0.0, -0.125],
         [dn, dn, THR, up, -up, 0.0, -0.0, THR, 0.75, -0.5, dn]]
    n = 40
    cols = spread_cols(n)
    db = one_hot(cols)
    q = np.zeros((len(V), DIM), np.float32)
    for i, v in enumerate(V):
        q[i, cols[:len(v)]] = np.asarray(v, np.float32)
    return db, q, np.asarray([v + [0.0] * (n - len(v)) for v in V], np.float32).T


TIE_COL, BG_COL = 3, 1000


def tie_case(n, groups):
    """n rows; group g = row indices that hold bit-identical copies of d_g = e_(TIE_COL + 2 g) + 0.5 e_BG_COL, query g = d_g (score 1.25 on its copies, 0.25 on
    other groups' copies).  Background rows alternate between e_BG_COL (score 0.5) and 0."""
    db = np.zeros((n, DIM), np.float32)
    db[0::2, BG_COL] = 1.0
    q = np.zeros((len(groups), DIM), np.float32)
    for g, rows in enumerate(groups):
        d = np.zeros(DIM, np.float32); d[TIE_COL + 2 * g] = 1.0; d[BG_COL] = 0.5
        for r in rows:
            assert 0 <= r < n
            db[r] = d
        q[g] = d
    assert len({r for rows in groups for r in rows}) == sum(len(rows) for rows in groups)
    return db, q


# pairs (first row, first row + offset): GEMM lane layout (+1 same lane next register, +4 other k-half lanes, +8, +32 other i, +64 other wave row, +128 next
# block) and GEMV layout (+1 same wave, +8 next wave, +32 next block); first rows sit at 1 mod 256 so that every offset lands where it says
TIE_OFFSETS = (1, 4, 8, 32, 64, 128)


def tie_groups(n, far_lo, far_hi):
    groups = [[256 * (j + 1) + 1, 256 * (j + 1) + 1 + off] for j, off in enumerate(TIE_OFFSETS)]
    groups.append([far_lo, far_hi])                          # 64 blocks apart: one lane of k_db_reduce holds both partials, or the higher block sits in the lower lane
    groups.append([2000, 2001, 2040])                        # three copies: a limit between them hides the upper ones
    assert max(max(g) for g in groups) < n
    return groups


def limit_case(n, limits):
    """n one-hot rows (ids 100 + 30 r: a cut-off window holds at most one id) and one query per limit p: the best row of the matrix is row p (score 4, just
    outside), the best row the scan sees is p - 1 (score 2), every other row scores (r mod 5) / 4, below and above thr_low.  cur puts the limit at p
    (p >= n: the whole matrix is seen)."""
    cols = spread_cols(n)
    db = one_hot(cols)
    ids = (100 + 30 * np.arange(n)).astype(np.uint64)
    q = np.zeros((len(limits), DIM), np.float32); cur = np.zeros(len(limits), np.uint64)
    for i, p in enumerate(limits):
        q[i, cols] = (np.arange(n) % 5) / 4.0
        if p < n:
            q[i, cols[p]] = 4.0
        if 1 <= p <= n:
            q[i, cols[p - 1]] = 2.0
        cur[i] = ids[p] + np.uint64(i % 20) if p < n else ids[-1] + np.uint64(20 + i)
    return db, ids, q, cur


LIMITS = (0, 1, 4, 8, 31, 32, 33, 64, 127, 128, 129)


def graded(n, nq):
    """query i gives one-hot row r the score ((3 r + i) mod 11) / 8: many equal scores, on both sides of thr_low"""
    cols = spread_cols(n)
    q = np.zeros((nq, DIM), np.float32)
    for i in range(nq):
        q[i, cols] = ((3 * np.arange(n) + i) % 11) / 8.0
    return one_hot(cols), q, cols


def owned_start_case(n=140):
    """One owned shard, ids 100 + 30 r.  Three queries per t of LIMITS: (a) cur just below ids[t] with an empty window: prefix [0, t), suffix [t, n), the
    best row of the matrix at t - 1 (the suffix must not see it), the suffix's best at t; (b) as (a) with equal scores at t - 1 and t; (c) cur = ids[t]:
    the window holds row t, suffix [t + 1, n).  The last query lies above every id: no suffix at all."""
    db, q, cols = graded(n, 3 * len(LIMITS) + 1)
    ids = (100 + 30 * np.arange(n)).astype(np.uint64)
    cur = np.zeros(len(q), np.uint64)
    for j, t in enumerate(LIMITS):
        for v in range(3):
            i = 3 * j + v
            if t >= 1:
                q[i, cols[t - 1]] = 4.0
            q[i, cols[t]] = 4.0 if v == 1 else 2.0
            cur[i] = ids[t] - np.uint64(5) if v < 2 else ids[t]
    cur[-1] = ids[-1] + np.uint64(25)
    return db, ids, q, cur


def owned_wrap_case(t0, small=()):
    """One owned shard whose last 19 ids are 2^64 - 19 .. 2^64 - 1, in rows t0 .. t0 + 18: a query with cur = c < 19 must stop in front of row t0 + c (the
    cut-off window wraps around 2^64).  The best row of the matrix sits there, the best row seen at t0 + c - 1.  `small` = ids below 19 at the front: queries at or
    above them break, and their suffix begins behind them.  Two more queries with cur >= 19 ride in the same call."""
    small = list(small)
    ids = np.array(small + [1000 + 30 * r for r in range(t0 - len(small))] + [M64 - 19 + j for j in range(19)], dtype=np.uint64)
    n = len(ids)
    db, q, cols = graded(n, 21)
    cur = np.zeros(21, np.uint64)
    for c in range(19):
        cur[c] = c
        q[c, cols[t0 + c]] = 4.0
        if t0 + c >= 1:
            q[c, cols[t0 + c - 1]] = 2.0
        for k, sid in enumerate(small):
            if sid <= c:
                q[c, cols[k]] = 8.0                           # better still, but at or below cur: in front of the suffix
    cur[19] = 1000 + 30 * 2 - 5; cur[20] = M64 - 1
    return db, ids, q, cur


def whole_map_case(n=300):
    """A whole map for the sharded tests: ids 100 + 30 r with the last five at 2^64 - 5 .. 2^64 - 1, graded scores with many ties, and queries whose cur lies
    inside a window, between windows, below 19, above everything and at 2^64 - 1"""
    ids = np.array([100 + 30 * r for r in range(n - 5)] + [M64 - 5 + j for j in range(5)], dtype=np.uint64)
    curs = [0, 3, 15, 18, 19, 20, 99, 100, 119, 120, M64 - 1, M64 - 3, M64 - 30, int(ids[n - 6]) + 19, int(ids[n - 6]) + 20, 10 ** 12]
    for p in LIMITS + (130, 200, 256, 257, n - 6):
        curs += [int(ids[p]), int(ids[p]) + 19, int(ids[p]) - 5]
    db, q, _ = graded(n, len(curs))
    return db, ids, q, np.array(curs, dtype=np.uint64)
