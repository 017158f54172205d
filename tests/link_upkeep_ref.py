"""The four rules that keep key-frame feature -> landmark links current on the device (include/myslam_hip.h, LINK UPKEEP), in plain Python:
culled_list (the list k_backend_write_back leaves), Store.clear_links (myslam_loop_store_clear_links_batch), filter_landmarks
(myslam_map_filter_landmarks_batch) and tracker_clear_links (myslam_tracker_clear_links_batch); and run_history, which holds them against
tests/whole_map_model.py: after every event of a history the gathered and filtered table of every stored key-frame must be what the object model says,
    key-frame k's feature i is linked iff its point is in all_mps and still has the Obs of that feature, otherwise -1.
A feature's index is its tag: the model's tags are unique over a history, and the store's feat_cap exceeds their number.  Test helper, no GPU."""
import numpy as np

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
import whole_map_model as wm

FEAT_CAP = 2048                 # above the tag count of every history of tests/test_whole_map_model.py (run_history asserts it)
CASES = ("culls_pending", "culls_stored", "entries_not_held", "erased_listed_links", "links_surviving")


def culled_list(t_in, obs_report):
    """the (key-frame id, tag) of every INPUT row with obs_report == 1, in row order.  t_in: the back end's tables before the call (backend_ref.pack)"""
    return [(int(t_in["kf_id"][t_in["obs_kf"][r]]), int(t_in["obs_tag"][r])) for r in range(len(t_in["obs_mp"])) if obs_report[r] == 1]


class Store:
    """myslam_loop_store as far as the links go: slot s holds the s-th key-frame put, ids ascend"""

    def __init__(self, feat_cap):
        self.feat_cap, self.ids, self.tables = int(feat_cap), [], []

    def put(self, kf_id, table, n_feat):
        assert not self.ids or kf_id > self.ids[-1]
        self.ids.append(int(kf_id))
        self.tables.append(np.array(table[:max(0, min(int(n_feat), self.feat_cap))], np.int32))

    def clear_links(self, entries, n=None, list_cap=None, pending_id=None, pending=None):
        """entries: [(kf id, tag)]; n: the device-side count (clamped to [0, list_cap]), None = all.  pending: the in/out table of the key-frame that is
        not put yet (changed in place).  -> the number of entries that named a stored or pending feature"""
        assert (pending_id is None) == (pending is None)
        if n is not None:
            entries = entries[:max(0, min(int(n), int(list_cap)))]
        hits = 0
        for kf_id, tag in entries:
            if kf_id < 0 or tag < 0:
                continue
            if pending is not None and kf_id == pending_id and tag < self.feat_cap:
                pending[tag] = -1
                hits += 1
            elif kf_id in self.ids:
                t = self.tables[self.ids.index(kf_id)]
                if tag < len(t):
                    t[tag] = -1
                    hits += 1
        return hits

    def gather(self, kf_id, fill=-1):
        """myslam_loop_detect_batch's d_loop_feat_landmark row: the stored entries, `fill` where the gather writes nothing"""
        row = np.full(self.feat_cap, fill, np.int32)
        t = self.tables[self.ids.index(kf_id)]
        row[:len(t)] = t
        return row


def filter_landmarks(row, mp_state):
    """-> (the row with every entry that names an erased point set to -1, the number of entries changed); mp_state: the archive's, n_mp long"""
    row = np.array(row, np.int32)
    drop = np.array([0 <= e < len(mp_state) and mp_state[e] == 2 for e in row.tolist()], bool)
    row[drop] = -1
    return row, int(drop.sum())


def tracker_clear_links(trk, entries, n=None, list_cap=None):
    """trk: dict(ids_valid, ref_frame_id, next_frame_id, ref_kf_id, lm: feature -> landmark slot, changed in place) -> entries that cleared a feature"""
    if not trk["ids_valid"] or trk["ref_frame_id"] != trk["next_frame_id"] - 1:
        return 0
    if n is not None:
        entries = entries[:max(0, min(int(n), int(list_cap)))]
    hits = 0
    for kf_id, tag in entries:
        if kf_id == trk["ref_kf_id"] and 0 <= tag < len(trk["lm"]):
            trk["lm"][tag] = -1
            hits += 1
    return hits


# ---------------------------------------------------------------------------------------------------------------------------------------------
# against the object model

def feat_ids_by_tag(feats, size=FEAT_CAP):
    """-> (map-point id by tag, -1 elsewhere; the feature count = the largest tag + 1): the d_feat_mp_id / d_n_feat a turn would write"""
    ids = np.full(size, -1, np.int64)
    for mid, _, _, tag, _ in feats:
        assert 0 <= tag < size
        ids[tag] = mid
    return ids, (max(f[3] for f in feats) + 1 if feats else 0)


def model_links(m, mp_ids, kf_id, feats, size=FEAT_CAP):
    """what mpMapPoint.lock() gives for every feature of key-frame kf_id in the model `m`, as archive slots by tag (mp_ids: the archive's ids)"""
    at = {int(v): i for i, v in enumerate(mp_ids)}
    row = np.full(size, -1, np.int32)
    for mid, _, _, tag, _ in feats:
        mp = m.all_mps.get(int(mid)) if mid >= 0 else None
        if mp is not None and any(o.tag == tag and int(o.kf) == kf_id for o in mp.obs):
            row[tag] = at[int(mid)]
    return row


def stored(n):
    """which key-frames of a history go into the store (the n-th one made): two of every five are left out on purpose"""
    return n % 5 not in (1, 3)


class Upkeep:
    """One history's store, the key-frames it holds and the case counters; the steps both the CPU test and the GPU test take on the model's side"""

    def __init__(self):
        self.feats = {}                             # key-frame id -> its features (every key-frame made, stored or not)
        self.order = []                             # key-frame ids in the order they were made
        self.seen = {k: 0 for k in CASES}
        self.listed_erased = set()                  # ids erased through the outlier list while observers still named them
        self.dropped_listed = set()                 # (key-frame, tag) of stored links the filter dropped for such an id

    def count_list(self, entries, pending_id, held):
        for kf_id, _ in entries:
            if kf_id == pending_id:
                self.seen["culls_pending"] += 1
            elif kf_id in held:
                self.seen["culls_stored"] += 1
            else:
                self.seen["entries_not_held"] += 1

    def note_erased(self, m, before_all, rep):
        """after m.optimize: the ids that left all_mps without having been emptied by the optimiser"""
        self.listed_erased |= {i for i in before_all if i not in m.all_mps and i not in rep["erased_by_ba"]}

    def check_rows(self, m, mp_ids, rows, filtered):
        """rows / filtered: key-frame id -> the gathered row before / after the filter, of every stored key-frame"""
        for kf_id, row in filtered.items():
            want = model_links(m, mp_ids, kf_id, self.feats[kf_id])
            assert np.array_equal(row, want), (kf_id, np.nonzero(row != want)[0][:5], row[row != want][:5], want[row != want][:5])
            for tag in np.nonzero(rows[kf_id] != row)[0].tolist():
                if int(mp_ids[rows[kf_id][tag]]) in self.listed_erased:
                    self.dropped_listed.add((kf_id, tag))
        self.seen["erased_listed_links"] = len(self.dropped_listed)
        self.seen["links_surviving"] = int(sum((r >= 0).sum() for r in filtered.values()))


def run_history(pkg, oracle, spec, K):
    """one history with the oracle's solve: the rules above on the walks' tables, the model beside them -> the case counters"""
    seed, window, n_kf, n_steps, extras = spec
    chain = pkg.chain
    m = wm.WholeMap(chain, window)
    w, a = br.Map(), mr.Archive()
    up, store = Upkeep(), Store(FEAT_CAP)
    pending = None
    frame = 0
    for ev in wm.history(seed, m, K, n_kf, n_steps, tuple(e for e in extras if e != "capacity")):
        if ev.kind == "correct":
            m.correct(ev.rigid, ev.moves)
            for k in w.kfs:
                w.kfs[k] = m.all_kfs[k].pose.copy()
            for i, mp in w.mps.items():
                mp.pos = m.all_mps[i].pos.copy()
            continue
        if ev.kind in ("insert", "refused"):
            ins = ev.ins
            ins.priors = m.priors_for(ins.feats)
            rw = mi.insert_walk(w, ins, window, 0.2, lambda pk, pn, row: m.dist(pk, pn))
            rm = m.insert_keyframe(ins)
            assert rw["status"] == rm["status"] == (mi.INVALID if ev.kind == "refused" else mi.OK)
            st = mr.update(chain, a, mr.AFTER_INSERT, br.pack(w), rw["status"], outlier_ids=ins.outlier_ids)
            assert st == (mr.SKIPPED if ev.kind == "refused" else mr.UPDATED)
            if ev.kind == "insert":
                pending = ins
                up.feats[ins.kf_id] = list(ins.feats); up.order.append(ins.kf_id)
                frame += 3
            continue
        assert ev.kind == "optimize"
        t_in = br.pack(w)
        sol = {}

        def solve(poses, pts, ep, el, eo, fixed):
            out = oracle.ba_optimize_active_map(poses, pts, ep, el, eo, fixed, K)
            sol["p"], sol["x"] = out[0], out[1]
            return out

        kf_ids = sorted(w.kfs)
        _, _, slot_mps = br.flatten(w) if br.validate(w) else (None, None, [])
        slot_ids = [mp.id for mp in slot_mps]
        before_all = set(m.all_mps)
        rw = br.walk(w, solve)
        rm = m.optimize(ev.flags, lambda: {k: sol["p"][i] for i, k in enumerate(kf_ids)}, lambda: {i: sol["x"][j] for j, i in enumerate(slot_ids)})
        assert rw["status"] == rm["status"]
        entries = []
        if rw["status"] == br.DONE:
            assert np.array_equal(rw["obs_report"], rm["obs_report"]), spec      # the oracle flags exactly the constructed outliers
            entries = culled_list(t_in, rw["obs_report"])
            assert len(entries) == rw["n_outlier_edges"] == len(ev.flags)
            up.note_erased(m, before_all, rm)
        st = mr.update(chain, a, mr.AFTER_OPTIMIZE, br.pack(w), rw["status"], mp_report=rw["mp_report"], left_pos=rw["left_pos"])
        assert st == (mr.UPDATED if rw["status"] == br.DONE else mr.SKIPPED)
        up.count_list(entries, pending.kf_id if pending else None, store.ids)
        if pending is not None:
            ids, n_feat = feat_ids_by_tag(pending.feats)
            assert n_feat <= FEAT_CAP
            table = mr.feature_slots(a, ids[:n_feat])
            table = np.concatenate([table, np.full(FEAT_CAP - n_feat, -1, np.int32)])
            # the tracker holds the same key-frame: its last frame is the key-frame's frame, feature -> landmark slot -> id
            lm_id = sorted({int(v) for v in ids[:n_feat] if v >= 0})
            trk = dict(ids_valid=1, ref_frame_id=frame, next_frame_id=frame + 1, ref_kf_id=pending.kf_id,
                       lm=np.array([lm_id.index(int(v)) if v >= 0 else -1 for v in ids[:n_feat]], np.int32))
            stepped = dict(trk, next_frame_id=frame + 2, lm=trk["lm"].copy())
            hits = store.clear_links(entries, pending_id=pending.kf_id, pending=table)
            t_hits = tracker_clear_links(trk, entries)
            assert tracker_clear_links(stepped, entries) == 0 and (stepped["lm"] >= 0).sum() == (ids[:n_feat] >= 0).sum()
            assert t_hits == sum(1 for k, _ in entries if k == pending.kf_id) <= hits
            # f.live() of StreamBank.hand_off: the feature's id, as far as culls go (an erased point needs no tracker rule: src/frontend.cpp:267)
            for mid, _, _, tag, _ in pending.feats:
                got = lm_id[trk["lm"][tag]] if trk["lm"][tag] >= 0 else -1
                mp = m.all_mps.get(int(mid)) if mid >= 0 else None
                culled = mid >= 0 and (pending.kf_id, tag) in entries
                assert got == (-1 if (mid < 0 or culled) else mid), (spec, pending.kf_id, tag)
                if mp is not None:                                           # alive: the tracker's link is the model's
                    assert (got >= 0) == any(o.tag == tag and int(o.kf) == pending.kf_id for o in mp.obs), (spec, pending.kf_id, tag)
            want = model_links(m, a.mp_id, pending.kf_id, pending.feats)
            assert np.array_equal(filter_landmarks(table, a.mp_state)[0], want), (spec, pending.kf_id)
            if stored(len(up.order) - 1):
                store.put(pending.kf_id, table, n_feat)
            pending = None
        else:
            store.clear_links(entries)
        rows = {k: store.gather(k) for k in store.ids}
        up.check_rows(m, a.mp_id, rows, {k: filter_landmarks(r, a.mp_state)[0] for k, r in rows.items()})
    assert len(up.order) == n_kf
    return up.seen
