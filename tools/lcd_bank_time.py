"""GPU timing of the loop database bank (csrc/lcd_bank.hip): S streams x R rows each, S in {16, 64, 256}, R in {100, 1000}.

Per shape: the time of one myslam_lcdbank_query_batch (three launches, every stream scanned: cur lies above every id) and of one
myslam_lcdbank_append_batch, and bytes of live rows (S * R * 4256) over the query time; and the time a caller needs for the same scans without the
bank — S myslam_lcddb_query_batch(nq = 1) calls on S single databases, one stream, host ids.  Both are host clocks around enqueued calls that end in
a device synchronise: 200 bank queries, 20 rounds of S single queries, 20 appends per window (an append stores a row, and the allocation is fixed).
Windows are repeated and the best and all values are kept.  Shapes of 272 MB and less are re-read out of the 256 MiB Infinity Cache from the second call
on: the JSON says which.

    python tools/lcd_bank_time.py [--out profiles/lcd_bank_time.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package(); api = pkg.api
DIM = api.LCD_DIM
WINDOWS, N = 5, 20
stream = torch.cuda.Stream()
out = {"tool": "tools/lcd_bank_time.py", "build_id": api.build_id(), "row_tile": api.LoopDatabaseBank.row_tile(),
       "launches_per_query": api.LoopDatabaseBank.launches_per_query(), "windows": WINDOWS, "calls_per_window": {"bank_query": 10 * N, "single_queries": N, "bank_append": N}, "shapes": {}}


def timed(fn, n=N):
    """ms per call: WINDOWS windows of n calls, each ended by a synchronise"""
    ms = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / n)
    return ms


rng = np.random.default_rng(3)
for S in (16, 64, 256):
    for R in (100, 1000):
        cap = R + (WINDOWS + 1) * N + 8
        rows = rng.standard_normal((R, DIM)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        ids = np.arange(R, dtype=np.uint64)
        with torch.cuda.stream(stream):
            bank = api.LoopDatabaseBank(S, cap, stream=stream.cuda_stream)
            singles = [api.LoopDatabase(R, stream=stream.cuda_stream) for _ in range(S)]
            d_rows = torch.from_numpy(rows).cuda()
            for s in range(S):
                bank.load(s, ids, np.roll(rows, s, axis=0))
                singles[s].append_batch(ids, torch.roll(d_rows, s, 0).contiguous().data_ptr(), R)
            q = torch.from_numpy(rows[rng.integers(0, R, S)].copy()).cuda()
            cur_host = np.full(S, R + 1000, np.uint64)
            cur = torch.from_numpy(cur_host.view(np.int64).copy()).cuda()
            best = torch.zeros(S, dtype=torch.int64, device="cuda"); mx = torch.zeros(S, device="cuda"); cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
            row = torch.zeros(S, dtype=torch.int32, device="cuda"); st = torch.zeros(S, dtype=torch.int32, device="cuda")
            best1 = torch.zeros(S, dtype=torch.int64, device="cuda"); mx1 = torch.zeros(S, device="cuda"); cnt1 = torch.zeros(S, dtype=torch.int32, device="cuda")
            new_id = torch.full((S,), R + 5, dtype=torch.int64, device="cuda")

            def bank_query():
                bank.query_batch(q.data_ptr(), cur.data_ptr(), 0, best.data_ptr(), mx.data_ptr(), cnt.data_ptr(), row.data_ptr(), st.data_ptr())

            def single_queries():
                for s in range(S):
                    singles[s].query_batch(q.data_ptr() + s * DIM * 4, cur_host[s:s + 1], 1, best1.data_ptr() + 8 * s, mx1.data_ptr() + 4 * s, cnt1.data_ptr() + 4 * s)

            def bank_append():
                new_id.add_(1)
                bank.append_batch(q.data_ptr(), new_id.data_ptr(), 0, st.data_ptr())

            for _ in range(3):
                bank_query(); single_queries()
            torch.cuda.synchronize()
            same = bool((best == best1).all() and (cnt == cnt1).all() and (st == 0).all())      # ids and counts of both paths (scores differ in the last bits: another order)
            tq, ts = [], []
            for _ in range(2):                                                 # alternating, so that both see the same machine
                tq += timed(bank_query, 10 * N); ts += timed(single_queries)
            ta = timed(bank_append)                                            # (the id bump is one more tiny launch per call, on both sides of no comparison)
            torch.cuda.synchronize()
            added_ok = bool((st == api.LCDBANK_ADDED).all())
        live = S * R * DIM * 4
        out["shapes"][f"S{S}_R{R}"] = {
            "streams": S, "rows_per_stream": R, "live_bytes": live, "fits_infinity_cache": live <= 256 * 2 ** 20,
            "bank_query_ms": [round(x, 4) for x in tq], "bank_query_best_ms": round(min(tq), 4), "bank_query_GBps": round(live / (min(tq) * 1e-3) / 1e9, 1),
            "bank_append_ms": [round(x, 4) for x in ta], "bank_append_best_ms": round(min(ta), 4),
            "single_queries_ms": [round(x, 4) for x in ts], "single_queries_best_ms": round(min(ts), 4),
            "single_over_bank": round(min(ts) / min(tq), 2), "same_ids_and_counts": same, "appends_added": added_ok}
        print(f"S{S}_R{R}", json.dumps(out["shapes"][f"S{S}_R{R}"]), flush=True)
        del bank, singles, d_rows, q
print(json.dumps(out))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
