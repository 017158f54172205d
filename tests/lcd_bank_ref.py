"""The loop database bank (csrc/lcd_bank.hip) as plain Python: per-stream lists of ids and rows, the gate of src/loopclosing.cpp:62, DetectLoop's scan
(lcddb_scan_ref.scan, :126-143) and AddToDatabase's rules (:651-659, the ascending-id rule and the fixed capacity of the device form).  Nothing here
looks at the device; tests/test_lcd_bank_ref.py pins it, tests/test_gpu_lcd_bank.py holds the kernels to it."""
import numpy as np

import lcddb_scan_ref as R

SCANNED, GATED, IDLE, ADDED = 0, 1, 2, 3           # MYSLAM_LCDBANK_*
ERR_INVALID, ERR_CAPACITY = -1, -3
EMPTY = (0, np.float32(0.0), 0, -1)                # best id, max score, cnt, best row of an item that scanned nothing


class Bank:
    def __init__(self, streams, rows_per_stream):
        self.S, self.cap = int(streams), int(rows_per_stream)
        self.ids = [[] for _ in range(self.S)]
        self.rows = [[] for _ in range(self.S)]        # f32 vectors

    def sizes(self):
        return [len(x) for x in self.ids]

    def load(self, s, ids, rows):
        ids = [int(i) for i in ids]
        assert len(ids) <= self.cap and all(a < b for a, b in zip(ids, ids[1:])) and len(rows) == len(ids)
        self.ids[s] = ids
        self.rows[s] = [np.array(r, np.float32) for r in rows]

    def scores(self, s, q):
        """the scores of stream s's rows against q; they must be f32 numbers as f64 sums (constructed inputs: exact in every f32 order)"""
        if not self.rows[s]:
            return np.zeros(0, np.float32)
        return R.exact32(R.scores64(np.stack(self.rows[s]), q)[0])[:, 0]

    def query(self, q, cur, active=None, thr_low=R.THR, min_size=0, scores=None):
        """-> per stream (best_id, max_score, cnt, best_row, status); `scores` (per stream, optional) replaces self.scores(s, q[s])"""
        out = []
        for s in range(self.S):
            if active is not None and not active[s]:
                out.append(EMPTY + (IDLE,))
                continue
            if len(self.ids[s]) <= min_size:                                   # _mvDatabase.size() > _mnDatabaseMinSize
                out.append(EMPTY + (GATED,))
                continue
            sc = self.scores(s, q[s]) if scores is None else np.asarray(scores[s], np.float32)
            best, mx, cnt = R.scan(sc, self.ids[s], cur[s], thr_low)
            row = self.ids[s].index(best) if float(mx) > 0 else -1            # ids are distinct: the winning id names its row
            out.append((best, mx, cnt, row, SCANNED))
        return out

    def append(self, descr, ids, add=None):
        """-> per stream status; a refused or idle item changes nothing"""
        st = []
        for s in range(self.S):
            if add is not None and not add[s]:
                st.append(IDLE)
            elif len(self.ids[s]) >= self.cap:
                st.append(ERR_CAPACITY)
            elif self.ids[s] and int(ids[s]) <= self.ids[s][-1]:
                st.append(ERR_INVALID)
            else:
                self.ids[s].append(int(ids[s])); self.rows[s].append(np.array(descr[s], np.float32))
                st.append(ADDED)
        return st

    def clear(self, flags):
        for s in range(self.S):
            if flags[s]:
                self.ids[s] = []; self.rows[s] = []


def as_arrays(results):
    """list of (best_id, max_score, cnt, best_row, status) -> arrays (u64, f32, i32, i32, i32)"""
    return (np.array([r[0] for r in results], np.uint64), np.array([r[1] for r in results], np.float32), np.array([r[2] for r in results], np.int32),
            np.array([r[3] for r in results], np.int32), np.array([r[4] for r in results], np.int32))
