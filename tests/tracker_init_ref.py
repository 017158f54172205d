"""StereoInit of the multi-stream tracker (include/myslam_hip.h, myslam_tracker_reset_stream / _init_masks / _init_batch) walked literally on
the state dicts of tests/tracker_ref.py.  Test infrastructure: tests/test_tracker_init_ref.py pins this walk against Chain(OracleBackend).grab()
on the stand-in sequence, tests/test_gpu_tracker_init.py checks the device against it with check_item().  LK's and the triangulation's outputs
are ARGUMENTS, as in tracker_kf_ref.

A stream is (st, ids): st = the dict of api.Tracker.get_frame() plus "why" (tracker_kf_ref.WHY_*) and optionally "overflow" and "image",
ids = the dict of api.Tracker.get_ids()."""
import numpy as np

from tracker_kf_ref import ERR_CAPACITY, NO_TURN, WHY_NONE
from tracker_ref import INITING, TRACKING_GOOD

INIT_RETRY = 2
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], float)
OUT_COUNTS = ("new_kf_id", "n_feat", "n_outlier_mp")
OUT_ROWS = ("feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags")
STATE_KEYS = ("xy", "lm", "lm_pos", "lm_outlier", "ref_pose", "ref_frame_id", "last_rel", "rel_motion", "next_frame_id", "status", "kf_every", "frozen",
              "outlier_list")


def created():
    """a stream as myslam_tracker_create leaves it: every byte 0 but `frozen`"""
    st = {"xy": np.zeros((0, 2), np.float32), "lm": np.zeros(0, np.int32), "lm_pos": np.zeros((0, 3)), "lm_outlier": np.zeros(0, np.uint8),
          "ref_pose": np.zeros(7), "ref_frame_id": 0, "last_rel": np.zeros((4, 4)), "rel_motion": np.zeros((4, 4)), "next_frame_id": 0,
          "status": INITING, "kf_every": 0, "frozen": 1, "outlier_list": np.zeros(0, np.int32), "why": WHY_NONE, "overflow": 0}
    return st, {"landmark_id": np.zeros(0, np.int64), "ref_kf_id": 0, "next_kf_id": 0, "next_mp_id": 0, "valid": 0}


def reset(st, next_frame_id=0, next_kf_id=0, next_mp_id=0, kf_every=0):
    """myslam_tracker_reset_stream: the created state with identities where a pose stands, and the given counters; a stored image stays"""
    if min(next_frame_id, next_kf_id, next_mp_id, kf_every) < 0:
        raise ValueError("negative counter")
    new, ids = created()
    new.update(ref_pose=IDENT.copy(), last_rel=np.eye(4), rel_motion=np.eye(4), next_frame_id=next_frame_id, kf_every=kf_every)
    if "image" in st:
        new["image"] = st["image"]
    return new, dict(ids, next_kf_id=next_kf_id, next_mp_id=next_mp_id)


def eligible(st):
    return bool(st["frozen"]) and st["status"] == INITING and st.get("why", WHY_NONE) == WHY_NONE and not st.get("overflow", 0)


def mask(rows, cols, st):
    """DetectFeatures' mask over an empty feature table (frontend.cpp:305-309) for an init-eligible stream, all 0 otherwise"""
    return np.full((rows, cols), 255 if eligible(st) else 0, np.uint8)


def _none(st, m, status, frame_id, n_right=0):
    return {"new_kf_id": -1, "n_feat": 0, "n_outlier_mp": 0,
            "report": np.array([status, frame_id, m, n_right, 0, len(st["lm"]), len(st["lm_pos"]), 0], np.int32)}


def _copy(st):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def init(st, ids, new_xy, right_xy, right_ok, tri_xyz, tri_ok, cap, lm_cap, init_good):
    """rules a - g from the ACCEPTED right tracks and triangulation (per feature; read only where the right status is set)
    -> (new st, new ids, outputs).  A stream that is not eligible, or does not fit, comes back as it went in."""
    new_xy = np.asarray(new_xy, np.float32).reshape(-1, 2)
    m = len(new_xy)
    if not eligible(st):
        return st, ids, _none(st, m, NO_TURN, st["next_frame_id"] - 1)
    fid = st["next_frame_id"]
    if m > cap:
        return st, ids, _none(st, m, ERR_CAPACITY, fid)
    right_ok = np.asarray(right_ok, bool)[:m]
    n_right = int(np.count_nonzero(right_ok))
    if n_right < init_good:                                # StereoInit returns false (:285-287): the Frame took its id, nothing else happened
        new = _copy(st)
        new["next_frame_id"] = fid + 1
        return new, ids, _none(st, m, INIT_RETRY, fid, n_right)
    next_mp, kf_id = int(ids["next_mp_id"]), int(ids["next_kf_id"])
    feat_id, feat_pos, lm = np.full(m, -1, np.int64), np.zeros((m, 3)), np.full(m, -1, np.int32)
    pos = []
    for i in range(m):                                     # BuildInitMap (:385-417): feature order, id and slot by rank among the successes
        if right_ok[i] and tri_ok[i]:
            lm[i] = len(pos); feat_id[i] = next_mp + len(pos)
            feat_pos[i] = np.asarray(tri_xyz[i], float)    # X itself: chain.build_init_map does not multiply by the identity pose
            pos.append(feat_pos[i])
    if len(pos) > lm_cap:
        return st, ids, _none(st, m, ERR_CAPACITY, fid, n_right)
    new = _copy(st)
    new.update(xy=new_xy.copy(), lm=lm, lm_pos=np.array(pos, float).reshape(-1, 3), lm_outlier=np.zeros(len(pos), np.uint8), ref_pose=IDENT.copy(),
               ref_frame_id=fid, next_frame_id=fid + 1, last_rel=np.eye(4), rel_motion=np.eye(4), status=TRACKING_GOOD, frozen=0, why=WHY_NONE,
               outlier_list=np.zeros(0, np.int32))
    nids = {"landmark_id": next_mp + np.arange(len(pos), dtype=np.int64), "ref_kf_id": kf_id, "next_kf_id": kf_id + 1, "next_mp_id": next_mp + len(pos),
            "valid": 1}
    out = {"new_kf_id": kf_id, "new_kf_pose": IDENT.copy(), "feat_mp_id": feat_id, "feat_mp_pos": feat_pos, "feat_uv": new_xy.copy(),
           "feat_tag": np.arange(m, dtype=np.int32), "feat_flags": np.zeros(m, np.uint8), "n_feat": m, "outlier_mp_id": np.zeros(0, np.int64),
           "n_outlier_mp": 0, "right_xy": np.asarray(right_xy, np.float32).reshape(-1, 2)[:m], "right_ok": right_ok,
           "report": np.array([0, fid, m, n_right, len(pos), m, len(pos), 0], np.int32)}
    return new, nids, out


def triangulate(ops, K, baseline, p0, right_xy, right_ok):
    """ops.triangulate_stereo on the features with a right match -> per-feature (xyz, ok) arrays"""
    m = len(p0)
    xyz, ok = np.zeros((m, 3)), np.zeros(m, bool)
    cand = [i for i in range(m) if right_ok[i]]
    if cand:
        p0, rx = np.asarray(p0, np.float32), np.asarray(right_xy, np.float32)
        x, o = ops.triangulate_stereo(p0[cand, 0], p0[cand, 1], rx[cand, 0], rx[cand, 1], K[0], K[1], K[2], K[3], baseline)
        xyz[cand], ok[cand] = x, np.asarray(o, bool)
    return xyz, ok


def init_with(ops, K, baseline, st, ids, left, right, new_xy, cap, lm_cap, init_good):
    """the whole init with ops.lk_track / ops.triangulate_stereo -> (new st, new ids, outputs, debug dict)"""
    new_xy = np.asarray(new_xy, np.float32).reshape(-1, 2)
    if not eligible(st) or len(new_xy) > cap:
        return init(st, ids, new_xy, None, None, None, None, cap, lm_cap, init_good) + ({},)
    if len(new_xy):
        nxt, ok, _ = ops.lk_track(left, right, new_xy, new_xy)          # every start point is the feature's own pixel (:350-352)
    else:
        nxt, ok = np.zeros((0, 2), np.float32), np.zeros(0, bool)
    ok = np.asarray(ok, bool)
    xyz, tok = triangulate(ops, K, baseline, new_xy, nxt, ok)
    post, nids, out = init(st, ids, new_xy, nxt, ok, xyz, tok, cap, lm_cap, init_good)
    post = dict(post, image=np.asarray(left))               # the head stored the left image, whatever the tail decides
    return post, nids, out, {"right_xy": nxt, "right_ok": ok, "tri_xyz": xyz, "tri_ok": tok}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_item(tag, post, pids, out, w_post, w_ids, w_out):
    """one stream of a finished init_batch (post / pids: get_frame / get_ids after it, out: the stream's rows of the thirteen outputs) against
    the walk's (w_post, w_ids, w_out), byte for byte; the state keys the walk does not carry (image) are the caller's"""
    rep = np.asarray(out["report"]).tolist()
    assert rep == w_out["report"].tolist(), f"{tag}: report {rep} vs {w_out['report'].tolist()}"
    for k in OUT_COUNTS:
        assert int(out[k]) == int(w_out[k]), f"{tag}: {k} {int(out[k])} vs {int(w_out[k])}"
    if rep[0] == 0:
        m = int(w_out["n_feat"])
        for k in OUT_ROWS:
            assert _same(out[k][:m], np.asarray(w_out[k], np.asarray(out[k]).dtype)), f"{tag}: {k}"
        assert _same(out["new_kf_pose"], w_out["new_kf_pose"]), f"{tag}: key-frame pose"
        ok = np.asarray(w_out["right_ok"], bool)
        assert _same(np.asarray(out["right_ok"][:m]).astype(bool), ok) and _same(out["right_xy"][:m][ok], w_out["right_xy"][ok]), f"{tag}: right tracks"
    for k in STATE_KEYS:
        assert _same(post[k], np.asarray(w_post[k], np.asarray(post[k]).dtype)), f"{tag}: state {k}: {post[k]!r} vs {w_post[k]!r}"
    for k in pids:
        assert _same(pids[k], np.asarray(w_ids[k], np.asarray(pids[k]).dtype)), f"{tag}: ids {k}: {pids[k]!r} vs {w_ids[k]!r}"
