"""The whole map of one stream (myslam_map_*, include/myslam_hip.h): Map::mmAllKeyFrames / mmAllMapPoints and KeyFrame::mpLastKF /
mRelativePoseToLastKF as plain Python lists, updated from the back end's tables after every insert and optimise by the rules of the header, walked
literally; the index inputs of myslam_loop_correct_batch, the write-back and the feature slots on the same lists; and the packers that turn a
backend_ref.Map or the objects of <pkg>/chain.py into the tables the update reads.  Test helper, no GPU.

`faults` switches single rules off: the stand-ins tests/test_map_archive_ref.py rehearses its checker on."""
import numpy as np

import backend_ref as br

AFTER_INSERT, AFTER_OPTIMIZE = 0, 1         # MYSLAM_MAP_AFTER_*
UPDATED, SKIPPED, INVALID, CAPACITY = 0, 1, -1, -3
FAULTS = ("no_promotion", "no_first_refresh", "edge_to_row0", "report_by_output_row")
# two more, rehearsed by tests/test_whole_map_model.py only (the rendered run of tests/test_map_archive_ref.py holds ONE point that tells the first from
# the rule, and none that tells the second): the shorter first-observer rule the header warns about ("the record stays when the front row has
# obs_kf = -1"), and the last instead of the lowest departed observer
MORE_FAULTS = ("front_record_stays", "last_departed_observer")
FIELDS = ("kf_id", "kf_pose", "edge_v0", "edge_v1", "meas", "mp_id", "mp_pos", "mp_first_kf", "mp_state", "snapshot", "mp_gone_kf", "mp_win_mask", "win_kf")


class Archive:
    def __init__(self):
        self.kf_id, self.kf_pose = [], []           # ascending mnKFId, Tcw (7)
        self.edge_v0, self.edge_v1, self.meas = [], [], []
        self.mp_id, self.mp_pos, self.mp_first_kf, self.mp_state = [], [], [], []
        self.snapshot = []                          # archive slot of every back-end map-point row as of the last update
        # what makes the first observer exact once key-frames leave the window (a row with obs_kf = -1 no longer says whose it is):
        self.mp_gone_kf = []                        # lowest archive row among the point's observers that left the window, -1 = none
        self.mp_win_mask = []                       # bit k: the point had a row on row k of the back end's key-frame table at the last update
        self.win_kf = []                            # archive row of every row of that key-frame table

    def arrays(self):
        """the tables in the dtypes and shapes of api.MapArchive.get"""
        return dict(kf_id=np.array(self.kf_id, np.int64), kf_pose=np.array(self.kf_pose, np.float64).reshape(-1, 7),
                    edge_v0=np.array(self.edge_v0, np.int32), edge_v1=np.array(self.edge_v1, np.int32), meas=np.array(self.meas, np.float64).reshape(-1, 7),
                    mp_id=np.array(self.mp_id, np.int64), mp_pos=np.array(self.mp_pos, np.float64).reshape(-1, 3),
                    mp_first_kf=np.array(self.mp_first_kf, np.int32), mp_state=np.array(self.mp_state, np.uint8),
                    snapshot=np.array(self.snapshot, np.int32), mp_gone_kf=np.array(self.mp_gone_kf, np.int32),
                    mp_win_mask=np.array(self.mp_win_mask, np.uint16), win_kf=np.array(self.win_kf, np.int32))


def same(a, b):
    """two dicts of arrays (Archive.arrays() / MapArchive.get()): equal byte for byte -> None, else the first field that differs"""
    for k in FIELDS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


def edge_meas(chain, new_pose, prev_pose):
    """mRelativePoseToLastKF as T[v0] * T[v1]^-1: the stated formula, chain.py's operations in its order"""
    return chain.p7_of(chain.mm(chain.T_of(np.asarray(new_pose, float)), chain.T_inv(chain.T_of(np.asarray(prev_pose, float)))))


def update(chain, a, mode, t, be_status, outlier_ids=(), mp_report=None, caps=None, faults=(), left_pos=None):
    """myslam_map_update_batch for one item.  t: the back end's tables after the call, unpadded (backend_ref.pack's kf_id, kf_pose, mp_id, mp_pos, obs_mp,
    obs_kf); caps = (kf_cap, edge_cap, point_cap) or None; left_pos = backend_ref.walk's (INPUT row -> the optimised position of a point that left the
    table alive: what myslam_map_attach_solve lets the device read), None = nothing attached.  `a` is changed in place unless the status is not UPDATED."""
    if be_status != 0:
        return SKIPPED
    kf_id = [int(v) for v in t["kf_id"]]; mp_id = [int(v) for v in t["mp_id"]]
    ins = mode == AFTER_INSERT
    k0 = sum(1 for v in kf_id if v <= a.kf_id[-1]) if a.kf_id else 0     # rows from k0 / m0 on are above the archive's last id
    m0 = sum(1 for v in mp_id if v <= a.mp_id[-1]) if a.mp_id else 0
    kf_at = {v: i for i, v in enumerate(a.kf_id)}; mp_at = {v: i for i, v in enumerate(a.mp_id)}
    if any(v not in kf_at for v in kf_id[:k0]) or any(v not in mp_at for v in mp_id[:m0]):
        return INVALID                              # an id at or below the archive's last that it does not hold
    new_k, new_m = len(kf_id) - k0, len(mp_id) - m0
    if not ins and (new_k or new_m or len(mp_id) > len(a.snapshot)):
        return INVALID
    new_e = new_k - (1 if (not a.kf_id and new_k) else 0)
    if caps is not None and (len(a.kf_id) + new_k > caps[0] or len(a.edge_v0) + new_e > caps[1] or len(a.mp_id) + new_m > caps[2]):
        return CAPACITY
    if ins:
        for k in range(k0, len(kf_id)):             # Map::InsertKeyFrame + mpLastKF / mRelativePoseToLastKF
            r = len(a.kf_id)
            if r > 0:
                v1 = 0 if "edge_to_row0" in faults else r - 1
                a.edge_v0.append(r); a.edge_v1.append(v1); a.meas.append(edge_meas(chain, t["kf_pose"][k], a.kf_pose[r - 1]))
            a.kf_id.append(kf_id[k]); a.kf_pose.append(np.array(t["kf_pose"][k], float))
        for m in range(m0, len(mp_id)):             # Map::InsertMapPoint
            a.mp_id.append(mp_id[m]); a.mp_pos.append(np.array(t["mp_pos"][m], float)); a.mp_first_kf.append(-1); a.mp_state.append(0)
            a.mp_gone_kf.append(-1); a.mp_win_mask.append(0)
        mp_at = {v: i for i, v in enumerate(a.mp_id)}
        for mid in outlier_ids:                     # Map::AddOutlierMapPoint
            s = mp_at.get(int(mid))
            if s is not None and a.mp_state[s] == 0:
                a.mp_state[s] = 1
    else:                                           # Map::RemoveAllOutlierMapPoints
        if "report_by_output_row" in faults:
            for m, mid in enumerate(mp_id):
                if mp_report[m] == 2:
                    a.mp_state[mp_at[mid]] = 2
        else:
            for m, s in enumerate(a.snapshot):
                if mp_report[m] == 2:
                    a.mp_state[s] = 2
        for m, s in enumerate(a.snapshot):          # SetPos (backend.cpp:259-261) before RemoveOldActiveMapPoints (map.cpp:126-140)
            if mp_report[m] == 1 and left_pos is not None and m in left_pos:
                a.mp_pos[s] = np.array(left_pos[m], float)
        if "no_promotion" not in faults:
            a.mp_state = [2 if s == 1 else s for s in a.mp_state]
    kf_at = {v: i for i, v in enumerate(a.kf_id)}
    for k, v in enumerate(kf_id):                   # refresh
        a.kf_pose[kf_at[v]] = np.array(t["kf_pose"][k], float)
    win = [kf_at[v] for v in kf_id]
    frozen = lambda s: "no_first_refresh" in faults and a.mp_first_kf[s] >= 0
    for s in a.snapshot:                            # the points of the table before the call: observers that left the window with this insert
        for k, row in enumerate(a.win_kf):
            if row not in win and (a.mp_win_mask[s] >> k) & 1:
                a.mp_gone_kf[s] = row if a.mp_gone_kf[s] < 0 else (max if "last_departed_observer" in faults else min)(a.mp_gone_kf[s], row)
        if a.mp_gone_kf[s] >= 0 and not frozen(s) and "front_record_stays" not in faults:  # a point that is leaving keeps only such rows: the lowest is its front
            a.mp_first_kf[s] = a.mp_gone_kf[s]
    for m, mid in enumerate(mp_id):
        s = mp_at[mid]
        a.mp_pos[s] = np.array(t["mp_pos"][m], float)
        rows = [int(k) for k in np.asarray(t["obs_kf"])[np.asarray(t["obs_mp"]) == m] if k >= 0]
        a.mp_win_mask[s] = sum(1 << k for k in set(rows))
        cand = [c for c in ([win[rows[0]]] if rows else []) + [a.mp_gone_kf[s]] if c >= 0]
        if "front_record_stays" in faults:          # the front row alone decides: a key-frame of the window is taken, -1 keeps what was recorded
            front = [int(k) for k in np.asarray(t["obs_kf"])[np.asarray(t["obs_mp"]) == m]][:1]
            cand = [win[front[0]]] if front and front[0] >= 0 else []
        if cand and not frozen(s):                  # both observation lists are in key-frame order: the front is the lowest row
            a.mp_first_kf[s] = min(cand)
    a.snapshot = [mp_at[mid] for mid in mp_id]
    a.win_kf = win
    return UPDATED


def loop_inputs(a, t, cur_kf_id, loop_kf_id, detect_status):
    """myslam_map_loop_inputs_batch for one item -> dict(active, cur, loop, first_active, first_kf, n_points); t as in update, with obs_flags"""
    if cur_kf_id < 0:
        return dict(active=np.zeros(0, np.int32), cur=-1, loop=-1, first_active=np.zeros(0, np.int32), first_kf=np.zeros(0, np.int32), n_points=0)
    kf_at = {v: i for i, v in enumerate(a.kf_id)}
    fa = np.full(len(a.mp_id), -1, np.int32)
    be_row = {int(v): m for m, v in enumerate(t["mp_id"])}
    for s, mid in enumerate(a.mp_id):
        m = be_row.get(mid)
        if m is not None:
            for r in np.nonzero(np.asarray(t["obs_mp"]) == m)[0]:
                if t["obs_flags"][r] & br.ACTIVE:
                    fa[s] = t["obs_kf"][r]
                    break
    fk = np.array([(-1 if st == 2 else f) for st, f in zip(a.mp_state, a.mp_first_kf)], np.int32)
    return dict(active=np.array([kf_at.get(int(v), -1) for v in t["kf_id"]], np.int32), cur=kf_at.get(int(cur_kf_id), -1),
                loop=(kf_at.get(int(loop_kf_id), -1) if detect_status == 0 else -1), first_active=fa, first_kf=fk, n_points=len(a.mp_id))


def feature_slots(a, feat_mp_id):
    at = {v: i for i, v in enumerate(a.mp_id)}
    return np.array([(at[int(v)] if (v >= 0 and int(v) in at and a.mp_state[at[int(v)]] != 2) else -1) for v in feat_mp_id], np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# <pkg>/chain.py's objects -> the back end's tables (what myslam_backend_* would hold for that Chain at that moment)

def pack_chain(c):
    """Chain's active map as the unpadded tables of myslam_backend_optimize_batch (kf_id, kf_pose, mp_id, mp_pos, obs_mp, obs_kf, obs_flags): every
    entry of GetObservations() of every active map point is a row, in list order"""
    kf_ids = sorted(c.active_kfs); row = {k: i for i, k in enumerate(kf_ids)}
    mp_ids = sorted(c.active_mps)
    obs_mp, obs_kf, obs_flags = [], [], []
    for m, mid in enumerate(mp_ids):
        mp = c.active_mps[mid]
        for f in mp.obs:
            obs_mp.append(m); obs_kf.append(row.get(f.kf.id, -1))
            obs_flags.append((br.ACTIVE if any(g is f for g in mp.active_obs) else 0) | (br.OUTLIER if f.outlier else 0))
    return dict(kf_id=np.array(kf_ids, np.int64), kf_pose=np.array([c.active_kfs[k].pose for k in kf_ids], np.float64).reshape(-1, 7),
                mp_id=np.array(mp_ids, np.int64), mp_pos=np.array([c.active_mps[i].pos for i in mp_ids], np.float64).reshape(-1, 3),
                obs_mp=np.array(obs_mp, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_flags=np.array(obs_flags, np.uint8))


def check_against_chain(a, c, erased_ids):
    """The archive against Chain's all_kfs / all_mps (`erased_ids`: every id Chain ever erased) -> None or what differs"""
    kfs = sorted(c.all_kfs)
    if a.kf_id != kfs:
        return "kf ids"
    for r, k in enumerate(kfs):
        if np.asarray(a.kf_pose[r], float).tobytes() != np.asarray(c.all_kfs[k].pose, float).tobytes():
            return "pose of key-frame %d" % k
    if [(v0, v1) for v0, v1 in zip(a.edge_v0, a.edge_v1)] != [(r, kfs.index(c.all_kfs[k].last_kf.id)) for r, k in enumerate(kfs) if c.all_kfs[k].last_kf is not None]:
        return "edge endpoints"
    alive = {mid for mid, st in zip(a.mp_id, a.mp_state) if st != 2}
    if alive != set(c.all_mps) or set(a.mp_id) != set(c.all_mps) | set(erased_ids):
        return "alive set: %s" % sorted(alive ^ set(c.all_mps))[:5]
    for s, mid in enumerate(a.mp_id):
        if a.mp_state[s] == 2:
            continue
        mp = c.all_mps[mid]
        if np.asarray(a.mp_pos[s], float).tobytes() != np.asarray(mp.pos, float).tobytes():
            return "position of map point %d" % mid
        if (a.mp_state[s] == 1) != (mid in c.outlier_mps):
            return "outlier list state of map point %d" % mid
        if mp.obs and kfs[a.mp_first_kf[s]] != mp.obs[0].kf.id:
            return "first observer of map point %d" % mid
    return None
