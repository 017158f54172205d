"""The key-frame turn of the multi-stream tracker (include/myslam_hip.h, myslam_tracker_keyframe_masks / _keyframe_batch /
_update_from_map_batch) walked literally on the state dicts of tests/tracker_ref.py with the SE3 helpers of <pkg>/chain.py.  Test infrastructure:
tests/test_tracker_kf_ref.py pins this walk against Chain(OracleBackend) at every key-frame of the stand-in sequence, tests/test_gpu_tracker_kf.py
checks the device against it.  LK's and the triangulation's outputs are ARGUMENTS (as tracker_ref.finish takes accepted outputs).

A stream is (st, ids): st = the dict of api.Tracker.get_frame() plus "why" (WHY_*: what the freezing step recorded), ids = the dict of
api.Tracker.get_ids() (landmark_id by slot, ref_kf_id, next_kf_id, next_mp_id, valid)."""
import numpy as np

WHY_NONE, WHY_KEYFRAME, WHY_LOST, WHY_CAPACITY = range(4)
NO_TURN, ERR_CAPACITY = 1, -3


def why_of(rec):
    """what the step's tail records for a result record"""
    if not rec["needs_host"]:
        return WHY_NONE
    if rec["status"] == ERR_CAPACITY:
        return WHY_CAPACITY
    return WHY_LOST if rec["status"] == 3 else WHY_KEYFRAME


def eligible(st, ids):
    return bool(st["frozen"]) and st.get("why", WHY_NONE) == WHY_KEYFRAME and bool(ids["valid"])


def cv_round(v):
    """cvRound of a float: nearest, ties to even"""
    return int(np.rint(np.float32(v)))


def mask(rows, cols, st, ids):
    """Frontend::DetectFeatures' mask (frontend.cpp:305-309) for an eligible stream, all 0 otherwise; a non-finite coordinate draws nothing"""
    if not eligible(st, ids):
        return np.zeros((rows, cols), np.uint8)
    m = np.full((rows, cols), 255, np.uint8)
    for x, y in np.asarray(st["xy"], np.float32).reshape(-1, 2):
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        x0, x1 = cv_round(x - np.float32(20)), cv_round(x + np.float32(20))
        y0, y1 = cv_round(y - np.float32(20)), cv_round(y + np.float32(20))
        m[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = 0
    return m


def world2pixel_right(chain, K, baseline, pw, Tcw):
    """chain.Chain.world2pixel(right=True)"""
    pc = chain.mv(Tcw[:3, :3], pw) + Tcw[:3, 3]
    pc = pc + np.array([-baseline, 0.0, 0.0])
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])


def Tcw_of(chain, st):
    return chain.mm(np.asarray(st["last_rel"], float), chain.T_of(st["ref_pose"]))


def append_and_starts(chain, K, baseline, st, new_xy):
    """rules a + b -> (left pixels of the final table, right start points, landmark of each feature)"""
    new_xy = np.asarray(new_xy, np.float32).reshape(-1, 2)
    p0 = np.concatenate([np.asarray(st["xy"], np.float32).reshape(-1, 2), new_xy])
    lm = np.concatenate([np.asarray(st["lm"], np.int32), np.full(len(new_xy), -1, np.int32)])
    Tcw = Tcw_of(chain, st)
    p1 = p0.copy()
    for i, l in enumerate(lm):
        if l >= 0 and not st["lm_outlier"][l]:
            p1[i] = world2pixel_right(chain, K, baseline, st["lm_pos"][l], Tcw).astype(np.float32)
    return p0, p1, lm


def candidates(lm, right_ok):
    """the features TriangulateNewPoints triangulates (frontend.cpp:456-460), in feature order"""
    return [i for i in range(len(lm)) if lm[i] < 0 and right_ok[i]]


def no_turn(st, n_new, status):
    return {"new_kf_id": -1, "n_feat": 0, "n_outlier_mp": 0,
            "report": np.array([status, st["next_frame_id"] - 1, n_new, 0, 0, len(st["lm"]), len(st["lm_pos"]), 0], np.int32)}


def turn(chain, K, baseline, st, ids, new_xy, right_xy, right_ok, tri_xyz, tri_ok, cap, lm_cap):
    """rules a - g from the ACCEPTED right tracks (per feature of the final table) and triangulation (per feature; read only at the candidates)
    -> (new st, new ids, outputs).  A stream without a turn comes back as it went in."""
    new_xy = np.asarray(new_xy, np.float32).reshape(-1, 2)
    n, n_new = len(st["lm"]), len(new_xy)
    if not eligible(st, ids):
        return st, ids, no_turn(st, n_new, NO_TURN)
    if n + n_new > cap:
        return st, ids, no_turn(st, n_new, ERR_CAPACITY)
    p0, _, lm = append_and_starts(chain, K, baseline, st, new_xy)
    m = n + n_new
    Tcw = Tcw_of(chain, st)
    Twc = chain.T_inv(Tcw)
    old_id, old_pos, old_outl = np.asarray(ids["landmark_id"], np.int64), np.asarray(st["lm_pos"], float).reshape(-1, 3), np.asarray(st["lm_outlier"], np.uint8)
    outlier_mp_id = np.array([old_id[l] for l in st["outlier_list"]], np.int64)          # read BEFORE the rebuild
    # d: new map points, ids by rank among the successes
    feat_id = np.array([old_id[l] if l >= 0 else -1 for l in lm], np.int64)
    feat_pos = np.array([old_pos[l] if l >= 0 else np.zeros(3) for l in lm], float).reshape(-1, 3)
    feat_outl = np.array([old_outl[l] if l >= 0 else 0 for l in lm], np.uint8)
    next_mp = int(ids["next_mp_id"])
    n_tri = 0
    for i in candidates(lm, right_ok):
        if tri_ok[i]:
            feat_id[i] = next_mp + n_tri; n_tri += 1
            feat_pos[i] = chain.mv(Twc[:3, :3], np.asarray(tri_xyz[i], float)) + Twc[:3, 3]
    # e: StreamBank.hand_off's table: slots in order of first reference
    slot, new_id, new_pos, new_outl = {}, [], [], []
    new_lm = np.full(m, -1, np.int32)
    for i in range(m):
        if feat_id[i] >= 0:
            if feat_id[i] not in slot:
                slot[feat_id[i]] = len(new_id); new_id.append(feat_id[i]); new_pos.append(feat_pos[i]); new_outl.append(feat_outl[i])
            new_lm[i] = slot[feat_id[i]]
    if len(new_id) > lm_cap:
        return st, ids, no_turn(st, n_new, ERR_CAPACITY)
    # f: InsertKeyFrame's pose lines
    kf_id = int(ids["next_kf_id"])
    pose = chain.p7_of(Tcw)
    new = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    new.update(xy=p0, lm=new_lm, lm_pos=np.array(new_pos, float).reshape(-1, 3), lm_outlier=np.array(new_outl, np.uint8), ref_pose=pose,
               ref_frame_id=st["next_frame_id"] - 1, last_rel=np.eye(4), frozen=0, why=WHY_NONE, outlier_list=np.zeros(0, np.int32))
    nids = {"landmark_id": np.array(new_id, np.int64), "ref_kf_id": kf_id, "next_kf_id": kf_id + 1, "next_mp_id": next_mp + n_tri, "valid": 1}
    out = {"new_kf_id": kf_id, "new_kf_pose": pose, "feat_mp_id": feat_id, "feat_mp_pos": feat_pos, "feat_uv": p0, "feat_tag": np.arange(m, dtype=np.int32),
           "feat_flags": np.zeros(m, np.uint8), "n_feat": m, "outlier_mp_id": outlier_mp_id, "n_outlier_mp": len(outlier_mp_id),
           "right_xy": np.asarray(right_xy, np.float32).reshape(-1, 2)[:m], "right_ok": np.asarray(right_ok, bool)[:m],
           "report": np.array([0, st["next_frame_id"] - 1, n_new, int(np.count_nonzero(np.asarray(right_ok)[:m])), n_tri, m, len(new_id), 0], np.int32)}
    return new, nids, out


def triangulate_candidates(ops, K, baseline, p0, right_xy, cand):
    """ops.triangulate_stereo on the candidates -> per-feature (xyz, ok) arrays"""
    m = len(p0)
    xyz, ok = np.zeros((m, 3)), np.zeros(m, bool)
    if cand:
        p0, rx = np.asarray(p0, np.float32), np.asarray(right_xy, np.float32)
        x, o = ops.triangulate_stereo(p0[cand, 0], p0[cand, 1], rx[cand, 0], rx[cand, 1], K[0], K[1], K[2], K[3], baseline)
        xyz[cand], ok[cand] = x, np.asarray(o, bool)
    return xyz, ok


def turn_with(chain, ops, K, baseline, st, ids, left, right, new_xy, cap, lm_cap):
    """the whole turn with ops.lk_track / ops.triangulate_stereo (the oracle's operators, or the product's single-image calls)
    -> (new st, new ids, outputs, debug dict)"""
    if not eligible(st, ids) or len(st["lm"]) + len(new_xy) > cap:
        return turn(chain, K, baseline, st, ids, new_xy, None, None, None, None, cap, lm_cap) + ({},)
    p0, p1, lm = append_and_starts(chain, K, baseline, st, new_xy)
    if len(p0):
        nxt, ok, _ = ops.lk_track(left, right, p0, p1)
    else:
        nxt, ok = np.zeros((0, 2), np.float32), np.zeros(0, bool)
    ok = np.asarray(ok, bool)
    cand = candidates(lm, ok)
    xyz, tok = triangulate_candidates(ops, K, baseline, p0, nxt, cand)
    return turn(chain, K, baseline, st, ids, new_xy, nxt, ok, xyz, tok, cap, lm_cap) + ({"p0": p0, "p1": p1, "lm": lm, "right_xy": nxt, "right_ok": ok,
                                                                                       "cand": cand, "tri_xyz": xyz, "tri_ok": tok},)


def update_from_map(st, ids, kf_id, kf_pose, mp_id, mp_pos, mp_outlier):
    """myslam_tracker_update_from_map_batch for one stream: a running stream with valid ids follows its ids; absent ids keep their values"""
    if st["frozen"] or not ids["valid"]:
        return st
    new = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    row = {int(i): r for r, i in enumerate(mp_id)}
    for l, i in enumerate(ids["landmark_id"]):
        if int(i) in row:
            new["lm_pos"][l] = mp_pos[row[int(i)]]; new["lm_outlier"][l] = mp_outlier[row[int(i)]]
    kf_row = {int(i): r for r, i in enumerate(kf_id)}
    if int(ids["ref_kf_id"]) in kf_row:
        new["ref_pose"] = np.array(kf_pose[kf_row[int(ids["ref_kf_id"])]], float)
    return new
