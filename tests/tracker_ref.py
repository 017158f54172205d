"""One step of the multi-stream tracker (include/myslam_hip.h, myslam_tracker_step_batch: rules 1 - 6) restated on plain arrays with the SE3
helpers of <pkg>/chain.py and the ORACLE's lk_track / pose_only_optimize.  Test infrastructure: tests/test_tracker_ref.py checks this
restatement frame by frame against Chain(OracleBackend).track(), tests/test_gpu_tracker.py checks the device against it in lock-step.
A state is the dict api.Tracker.get_frame() returns (xy, lm, lm_pos, lm_outlier, ref_pose, ref_frame_id, last_rel, rel_motion,
next_frame_id, status, kf_every, frozen, outlier_list)."""
import numpy as np

INITING, TRACKING_GOOD, TRACKING_BAD, LOST = range(4)


def world2pixel(chain, K, pw, Tcw):
    pc = chain.mv(Tcw[:3, :3], pw) + Tcw[:3, 3]
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])


def predict(chain, K, st):
    """rule 1 -> (cur.rel, p0, p1)"""
    Tref = chain.T_of(st["ref_pose"])
    rel = chain.mm(st["rel_motion"], st["last_rel"])
    Tcw = chain.mm(rel, Tref)
    p0 = np.array(st["xy"], np.float32).reshape(-1, 2)
    p1 = p0.copy()
    for i, l in enumerate(st["lm"]):
        if l >= 0 and not st["lm_outlier"][l]:
            p1[i] = world2pixel(chain, K, st["lm_pos"][l], Tcw).astype(np.float32)
    return rel, p0, p1


def compact(st, nxt, lk_st):
    """rule 3 -> (current feature table xy, lm; for each of its features the row of the pose-only problem or -1)"""
    keep = [i for i in range(len(st["lm"])) if lk_st[i] and st["lm"][i] >= 0]
    xy = np.array([nxt[i] for i in keep], np.float32).reshape(-1, 2)
    lm = np.array([st["lm"][i] for i in keep], np.int32)
    po, k = [], 0
    for l in lm:
        if st["lm_outlier"][l]:
            po.append(-1)
        else:
            po.append(k); k += 1
    return xy, lm, np.array(po, np.int32)


def finish(chain, st, xy, lm, po, pose, outl, n_inl, good, bad):
    """rules 5 + 6 from the ACCEPTED pose / flags / inlier count -> (new state, result record)"""
    new = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    fid = st["next_frame_id"]
    lm = lm.copy()
    lst = list(st.get("outlier_list", []))
    for j in range(len(lm)):
        if po[j] >= 0 and outl[po[j]]:
            if fid - st["ref_frame_id"] <= 2:
                new["lm_outlier"][lm[j]] = 1
                lst.append(int(lm[j]))
            lm[j] = -1
    Tref = chain.T_of(st["ref_pose"])
    rel = chain.mm(chain.T_of(pose), chain.T_inv(Tref))
    status = TRACKING_GOOD if n_inl > good else (TRACKING_BAD if n_inl > bad else LOST)
    new["rel_motion"] = chain.mm(rel, chain.T_inv(st["last_rel"]))
    new["last_rel"] = rel
    kfe = st.get("kf_every", 0)
    insert = status == TRACKING_BAD if kfe <= 0 else (status != LOST and fid % kfe == 0)
    needs = int(insert or status == LOST)
    new.update(xy=xy, lm=lm, status=status, next_frame_id=fid + 1, frozen=needs, outlier_list=np.array(lst, np.int32))
    rec = {"pose7": chain.p7_of(chain.mm(rel, Tref)), "n_inliers": int(n_inl), "n_features": len(lm), "status": status, "frame_id": fid, "needs_host": needs}
    return new, rec


def step(chain, oracle, K, st, prev_img, cur_img, good, bad):
    """the whole step with the oracle's operators -> (new state, record, debug dict)"""
    rel, p0, p1 = predict(chain, K, st)
    if len(p0):
        nxt, lk_st, _ = oracle.lk_track(prev_img, cur_img, p0, p1)
    else:
        nxt, lk_st = np.zeros((0, 2), np.float32), np.zeros(0, bool)
    xy, lm, po = compact(st, nxt, lk_st)
    sel = po >= 0
    p3 = np.array([st["lm_pos"][l] for l in lm[sel]], float).reshape(-1, 3)
    obs = xy[sel].astype(np.float64).reshape(-1, 2)
    pose0 = chain.p7_of(chain.mm(rel, chain.T_of(st["ref_pose"])))
    pose, outl, n_inl = oracle.pose_only_optimize(pose0, p3, obs, K)
    new, rec = finish(chain, st, xy, lm, po, pose, outl, n_inl, good, bad)
    dbg = {"p0": p0, "p1": p1, "nxt": nxt, "lk_status": np.asarray(lk_st, bool), "xy": xy, "lm": lm, "po": po, "pose0": pose0, "p3": p3, "obs": obs,
           "pose": pose, "outlier": np.asarray(outl, bool), "n_inliers": int(n_inl)}
    return new, rec, dbg


def state_of_chain(chain, c, kf_every=0):
    """the state of a Chain whose current frame has just become `last` (after grab()): (state, landmark ids by slot)"""
    feats = c.cur.feats
    ids, slot = [], {}
    lm = np.full(len(feats), -1, np.int32)
    for i, f in enumerate(feats):
        mp = f.live()
        if mp is not None:
            if mp.id not in slot:
                slot[mp.id] = len(ids); ids.append(mp.id)
            lm[i] = slot[mp.id]
    st = {"xy": np.array([[f.x, f.y] for f in feats], np.float32).reshape(-1, 2), "lm": lm,
          "lm_pos": np.array([c.all_mps[m].pos for m in ids], float).reshape(-1, 3),
          "lm_outlier": np.array([1 if c.all_mps[m].outlier else 0 for m in ids], np.uint8),
          "ref_pose": np.array(c.ref_kf.pose, float), "ref_frame_id": c.ref_kf.frame_id, "last_rel": np.array(c.cur.rel, float),
          "rel_motion": np.array(c.rel_motion, float), "next_frame_id": c.next_frame_id, "status": c.status, "kf_every": kf_every, "frozen": 0,
          "outlier_list": np.zeros(0, np.int32)}
    return st, ids
