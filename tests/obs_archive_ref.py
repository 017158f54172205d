"""myslam_obs_archive_update_batch / _prior_rows_batch (include/myslam_hip.h, OBSERVATION ARCHIVE) as a table-shaped walk in plain Python: the mirror of
the back end's table with the observer's mnKFId of every row, the pool of stored segments with its bump pointer, the reclaim into the other pool.
It reads what the device reads: the back end's tables after the call (backend_ref.pack's dict, or an item cut out of the device's), the map archive
after ITS update (map_archive_ref.Archive: ids and states), the two statuses and after an optimise d_obs_report by INPUT row.  Test helper, no GPU."""
import numpy as np

import backend_ref as br

AFTER_INSERT, AFTER_OPTIMIZE = 0, 1
UPDATED, SKIPPED, OK, INVALID, CAPACITY = 0, 1, 0, -1, -3
FAULTS = ("keeps_culled_rows", "kf_id_from_wrong_rank", "returned_segment_stays")
GET_FIELDS = ("seg_mp_id", "seg_count", "row_kf_id", "row_uv", "row_tag", "row_flags", "table_mp_id", "table_mp_rows", "table_kf_id", "table_uv", "table_tag",
              "table_flags")


class Store:
    """one item.  A row is (mnKFId, u f32, v f32, tag, flags)."""

    def __init__(self, row_cap=1 << 20):
        self.row_cap = int(row_cap)
        self.pools = [{}, {}]               # row index -> row
        self.pcur, self.used, self.n_reclaim, self.err = 0, 0, 0, 0
        self.seg = {}                       # map-point id -> (offset, count), count 0 = nothing stored; the device keys it by the map's slot
        self.t_id, self.t_rows = [], []     # the mirror: the table's map-point ids and the rows of each
        self.seen = dict(left_insert=0, left_optimize=0, left_optimize_culled=0, returned=0, left_again=0, erased=0, longest=0, most_live=0)
        self._ever, self._again, self._was_live = set(), set(), set()

    @classmethod
    def loaded(cls, row_cap, segments, t_id, t_rows):
        """what myslam_obs_archive_load leaves: segments [(id ascending, rows)] packed from row 0 of pool 0, the mirror as given"""
        st = cls(row_cap)
        for mid, rows in segments:
            for j, r in enumerate(rows):
                st.pools[0][st.used + j] = tuple(r)
            st.seg[int(mid)] = (st.used, len(rows)); st.used += len(rows)
        st.t_id, st.t_rows = [int(i) for i in t_id], [[tuple(r) for r in rs] for rs in t_rows]
        return st

    def load_args(self, a):
        """the arguments of api.ObsArchive.load for this state"""
        x = self.arrays(a)
        return [x[k] for k in GET_FIELDS]

    def clone(self):
        import copy
        return copy.deepcopy(self)

    def live(self, a):
        """[(id, rows)] of the segments that are visible: stored, and alive in the map"""
        state = dict(zip(a.mp_id, a.mp_state))
        pool = self.pools[self.pcur]
        return [(mid, [pool[o + j] for j in range(c)]) for mid, (o, c) in sorted(self.seg.items()) if c > 0 and state.get(mid, 2) != 2]

    def arrays(self, a):
        """what api.ObsArchive.get returns"""
        live = self.live(a)
        rows = [r for _, rs in live for r in rs]
        trows = [r for rs in self.t_rows for r in rs]
        cols = lambda rs: (np.array([r[0] for r in rs], np.int64), np.array([(r[1], r[2]) for r in rs], np.float32).reshape(-1, 2),
                           np.array([r[3] for r in rs], np.int32), np.array([r[4] for r in rs], np.uint8))
        rk, ru, rt, rf = cols(rows)
        tk, tu, tt, tf = cols(trows)
        return dict(seg_mp_id=np.array([m for m, _ in live], np.int64), seg_count=np.array([len(rs) for _, rs in live], np.int32), row_kf_id=rk, row_uv=ru,
                    row_tag=rt, row_flags=rf, table_mp_id=np.array(self.t_id, np.int64), table_mp_rows=np.array([len(rs) for rs in self.t_rows], np.int32),
                    table_kf_id=tk, table_uv=tu, table_tag=tt, table_flags=tf, rows_in_use=self.used, n_reclaims=self.n_reclaim, error=self.err)


def same(got, want):
    """-> None or the name of the first field that differs (bytes and dtypes; the three counters as numbers)"""
    for k in GET_FIELDS:
        x, y = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return next((k for k in ("rows_in_use", "n_reclaims", "error") if int(got[k]) != int(want[k])), None)


def _segments(t):
    """the table's rows per map point: [(kf row or -1, u, v, tag, flags & OUTLIER)]"""
    out = [[] for _ in t["mp_id"]]
    for r, m in enumerate(t["obs_mp"]):
        out[int(m)].append((int(t["obs_kf"][r]), np.float32(t["obs_uv"][r][0]), np.float32(t["obs_uv"][r][1]), int(t["obs_tag"][r]),
                            int(t["obs_flags"][r]) & br.OUTLIER))
    return out


def update(st, mode, t, be_status, map_status, a, obs_report=None, faults=()):
    """one item's k_obs_update -> status.  `a`: the map archive after its update of the same call"""
    if st.err:
        return st.err
    if be_status != 0 or map_status == SKIPPED:
        return SKIPPED
    if map_status != UPDATED or len(t["kf_id"]) < 1:
        st.err = INVALID
        return INVALID
    ins = mode == AFTER_INSERT
    state = dict(zip(a.mp_id, a.mp_state))
    pool = st.pools[st.pcur]
    now = [int(i) for i in t["mp_id"]]
    segs = _segments(t)
    prev = {mid: p for p, mid in enumerate(st.t_id)}
    new_row = len(t["kf_id"]) - 1
    new_kf = int(t["kf_id"][-1])
    kept_rows = lambda p: [r for j, r in enumerate(st.t_rows[p]) if ins or obs_report[off[p] + j] != 1]
    off = np.concatenate([[0], np.cumsum([len(rs) for rs in st.t_rows])]).astype(int)
    stored = lambda mid: st.seg.get(mid, (0, 0))[1] if state.get(mid, 2) != 2 else 0
    # ---- decide
    bad = False
    for m, mid in enumerate(now):
        if mid not in state:
            bad = True
        elif mid in prev:
            old = len(st.t_rows[prev[mid]])
            bad |= len(segs[m]) < old if ins else len(segs[m]) != len(kept_rows(prev[mid]))
        elif ins:
            lead = next((j for j, r in enumerate(segs[m]) if r[0] == new_row), len(segs[m]))
            bad |= lead != stored(mid)
        else:
            bad = True
    leaving = [mid for mid in st.t_id if mid not in now]
    bad |= any(mid not in state for mid in leaving)
    if bad:
        st.err = INVALID
        return INVALID
    to_store = [(mid, kept_rows(prev[mid]) if "keeps_culled_rows" not in faults else list(st.t_rows[prev[mid]])) for mid in leaving if state[mid] != 2]
    keep = sum(c for mid, (o, c) in st.seg.items() if c > 0 and state.get(mid, 2) != 2 and mid not in now)
    n_leave = sum(len(rs) for _, rs in to_store)
    if keep + n_leave > st.row_cap:
        st.err = CAPACITY
        return CAPACITY
    # ---- write: the mirror
    t_rows = []
    for m, mid in enumerate(now):
        if mid in prev:
            if "kf_id_from_wrong_rank" in faults and not ins:
                src = list(st.t_rows[prev[mid]])[:len(segs[m])]
            else:
                src = kept_rows(prev[mid])
        else:
            o, c = st.seg.get(mid, (0, 0))
            src = [pool[o + j] for j in range(stored(mid))]
            if src:
                st.seen["returned"] += 1
            if "returned_segment_stays" not in faults:
                st.seg[mid] = (o, 0)
        t_rows.append([((src[j][0] if j < len(src) else new_kf),) + r[1:] for j, r in enumerate(segs[m])])
    # ---- the pool: reclaim when the append would not fit, then the leaving points in the recorded table's order
    if st.used + n_leave > st.row_cap:
        dst, base = {}, 0
        for mid, (o, c) in sorted(st.seg.items()):
            if c > 0 and state.get(mid, 2) != 2:
                for j in range(c):
                    dst[base + j] = pool[o + j]
                st.seg[mid] = (base, c); base += c
        st.pcur ^= 1
        st.pools[st.pcur] = pool = dst
        st.used = base
        st.n_reclaim += 1
    for mid, rs in to_store:
        if rs:
            for j, r in enumerate(rs):
                pool[st.used + j] = r
            st.seg[mid] = (st.used, len(rs)); st.used += len(rs)
            st.seen["left_insert" if ins else "left_optimize"] += 1
            if not ins and len(rs) < len(st.t_rows[prev[mid]]):
                st.seen["left_optimize_culled"] += 1
            st.seen["left_again"] += mid in st._ever and mid not in st._again        # points, not departures
            (st._again if mid in st._ever else st._ever).add(mid)
            st.seen["longest"] = max(st.seen["longest"], len(rs))
    st.t_id, st.t_rows = now, t_rows
    live = {mid for mid, _ in st.live(a)}
    st.seen["erased"] += sum(1 for mid in st._was_live if mid not in live and mid not in now and state.get(mid, 2) == 2)
    st._was_live = live
    st.seen["most_live"] = max(st.seen["most_live"], sum(st.seg[mid][1] for mid in live))
    return UPDATED


def prior_rows(st, feat_ids, table_mp_id, a, prior_cap=1 << 20):
    """one item's k_obs_prior_rows -> (status, [(map-point id, mnKFId, (u, v), tag, outlier)]) in the form of map_insert_ref.Insert.priors"""
    if st.err:
        return st.err, []
    state = dict(zip(a.mp_id, a.mp_state))
    table = set(int(i) for i in table_mp_id)
    pool = st.pools[st.pcur]
    ids = sorted({int(i) for i in feat_ids if i >= 0 and int(i) not in table and state.get(int(i), 2) != 2 and st.seg.get(int(i), (0, 0))[1] > 0})
    rows = [(mid,) + pool[st.seg[mid][0] + j] for mid in ids for j in range(st.seg[mid][1])]
    if len(rows) > prior_cap:
        return CAPACITY, []
    return OK, [(mid, kf, (u, v), tag, bool(fl & br.OUTLIER)) for mid, kf, u, v, tag, fl in rows]


def same_priors(got, want):
    """two prior lists in the form of Insert.priors / whole_map_model.priors_for: ids, key-frame ids, f32 pixel bits, tags, outlier bits"""
    key = lambda p: (int(p[0]), int(p[1]), np.float32(p[2][0]).tobytes(), np.float32(p[2][1]).tobytes(), int(p[3]), bool(p[4]))
    return [key(p) for p in got] == [key(p) for p in want]
