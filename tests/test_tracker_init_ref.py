"""tests/tracker_init_ref.py (StereoInit of the multi-stream tracker walked on plain arrays) is itself checked: beside Chain(OracleBackend).grab()
on the stand-in sequence it reproduces the detection mask, the feature table, the right start points, BuildInitMap's map points, the key-frame
of InsertKeyFrame's INITING branch and the arrays StreamBank.hand_off would upload (taken before the back end runs) — on the first frame, and
on a run whose numFeatures.initGood lies above the match count for three frames, so that frames 0..2 retry and the frame ids still advance.
Then the GPU test's checker is rehearsed on faulty stand-ins of a device.  CPU only."""
import numpy as np
import pytest

import tracker_init_ref as IR
import tracker_kf_ref as KR
import tracker_ref as TR
from oracle_backend import OracleBackend

CFG = {"numFeatures.trackingGood": 390}
CAP, LM_CAP = 4096, 8192


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _chain(pkg, synth, oracle, n, cfg):
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(n)]
    c = chain.Chain(OracleBackend(oracle, synth.calc_weights_handcrafted(), cfg, chain), pkg.api, synth.SEQ_K, frames, cfg=cfg)
    seen = {}
    detect, backend = c.be.detect, c.backend_new_keyframe

    def spy_detect(img, mask, init):
        seen["mask"], seen["init"] = mask.copy(), init
        return detect(img, mask, init)

    def spy_backend(kf):                                  # InsertKeyFrame's frontend half is done; the back end has not run
        seen["handoff"] = TR.state_of_chain(chain, c)
        seen["kf"] = (kf.id, np.array(kf.pose), kf.frame_id, c.next_kf_id, c.next_mp_id)
        seen["feat_ids"] = [(f.mp.id if f.live() is not None else -1) for f in kf.feats]
        return backend(kf)

    c.be.detect, c.backend_new_keyframe = spy_detect, spy_backend
    return c, frames, seen


def _walk_frame(c, frames, seen, t, st, ids):
    """one grab() of an INITING chain beside the walk -> (post, ids, out, the chain's new log entries)"""
    n_log = len(c.log)
    rows, cols = frames[t][0].shape
    assert c.grab(t)
    log = {k: v for k, v in c.log[n_log:]}
    assert seen["init"] is True and _same(seen["mask"], IR.mask(rows, cols, st)) and seen["mask"].min() == 255, "mask over an empty table, init extractor"
    kps = log["detect"][0]
    new_xy = np.stack([kps["x"], kps["y"]], 1).astype(np.float32)
    nxt, ok, p1 = log["lk_right"]
    assert _same(p1, new_xy), "every right start point is the feature's own pixel"
    ok = np.asarray(ok, bool)
    xyz, tok = np.zeros((len(new_xy), 3)), np.zeros(len(new_xy), bool)
    if "triangulate" in log:
        cand = [i for i in range(len(ok)) if ok[i]]
        tok[cand] = np.asarray(log["triangulate"][0], bool)
        xyz[[i for i in cand if tok[i]]] = log["triangulate"][1]
    return IR.init(st, ids, new_xy, nxt, ok, xyz, tok, CAP, LM_CAP, c.n_init_good) + (log,)


def _check_against_handoff(chain, c, seen, post, nids, out, frame_id, kf_id):
    want, wids = seen["handoff"]
    got_kf, kf_pose, kf_frame, next_kf, next_mp = seen["kf"]
    assert out["report"][0] == 0 and out["new_kf_id"] == got_kf == kf_id and _same(out["new_kf_pose"], kf_pose) and _same(kf_pose, chain.IDENT)
    assert kf_frame == frame_id == out["report"][1] == post["ref_frame_id"]
    assert (nids["ref_kf_id"], nids["next_kf_id"], nids["next_mp_id"], nids["valid"]) == (got_kf, next_kf, next_mp, 1)
    assert seen["feat_ids"] == out["feat_mp_id"].tolist() and nids["landmark_id"].tolist() == wids
    feats = c.all_kfs[got_kf].feats
    assert _same(np.array([[f.x, f.y] for f in feats], np.float32), out["feat_uv"]) and out["n_feat"] == len(feats) == out["report"][2]
    for k in ("xy", "lm", "lm_pos", "lm_outlier", "ref_pose", "last_rel", "rel_motion"):
        assert np.asarray(want[k]).dtype == np.asarray(post[k]).dtype and _same(want[k], post[k]), "hand-off " + k
    assert (want["ref_frame_id"], want["next_frame_id"]) == (post["ref_frame_id"], post["next_frame_id"])
    assert want["status"] == TR.INITING, "the spy looks before StereoInit's status line (:291); grab() has run it since:"
    assert post["status"] == TR.TRACKING_GOOD == c.status and post["frozen"] == 0 and len(post["outlier_list"]) == 0 and not IR.eligible(post)
    assert all(_same(post["lm_pos"][post["lm"][i]], out["feat_mp_pos"][i]) for i in range(len(feats)) if post["lm"][i] >= 0)
    assert out["report"][4] == len(post["lm_pos"]) == len(c.all_mps) > 50 and out["report"][3] >= out["report"][4]


def test_walk_reproduces_stereo_init_on_the_first_frame(pkg, synth, oracle):
    c, frames, seen = _chain(pkg, synth, oracle, 1, CFG)
    st, ids = IR.created()
    assert IR.eligible(st)
    post, nids, out, _ = _walk_frame(c, frames, seen, 0, st, ids)
    _check_against_handoff(pkg.chain, c, seen, post, nids, out, 0, 0)
    # the same from a reset stream: identities where the created state holds zeros, and nothing of that reaches the result
    rst, rids = IR.reset(st)
    assert IR.eligible(rst) and _same(rst["rel_motion"], np.eye(4)) and _same(rst["ref_pose"], IR.IDENT)
    c2, frames2, seen2 = _chain(pkg, synth, oracle, 1, CFG)
    post2, nids2, out2, _ = _walk_frame(c2, frames2, seen2, 0, rst, rids)
    IR.check_item("reset", post2, nids2, out2, post, nids, out)


def test_walk_retries_while_matches_are_short_and_frame_ids_advance(pkg, synth, oracle):
    chain = pkg.chain
    c, frames, seen = _chain(pkg, synth, oracle, 4, dict(CFG, **{"numFeatures.initGood": 100000}))
    st, ids = IR.reset(IR.created()[0], next_frame_id=0, next_kf_id=5, next_mp_id=900, kf_every=3)
    c.next_kf_id, c.next_mp_id = 5, 900                   # a restart, or an id space shared with other streams
    for t in range(3):
        post, nids, out, log = _walk_frame(c, frames, seen, t, st, ids)
        assert c.status == chain.INITING and "handoff" not in seen and c.next_frame_id == t + 1 and _same(c.poses[-1], chain.IDENT)
        assert out["report"].tolist() == [IR.INIT_RETRY, t, len(log["detect"][0]), int(np.count_nonzero(log["lk_right"][1])), 0, 0, 0, 0]
        assert (out["new_kf_id"], out["n_feat"], out["n_outlier_mp"]) == (-1, 0, 0) and nids is ids and IR.eligible(post)
        assert post["next_frame_id"] == t + 1 and all(_same(post[k], st[k]) for k in IR.STATE_KEYS if k != "next_frame_id")
        st = post
    n_right = int(out["report"][3])
    c.n_init_good = n_right + 1                           # one short: still a retry ...
    assert IR.init(st, ids, np.zeros((n_right, 2)), np.zeros((n_right, 2)), np.ones(n_right, bool), np.zeros((n_right, 3)), np.zeros(n_right, bool),
                   CAP, LM_CAP, c.n_init_good)[2]["report"][0] == IR.INIT_RETRY
    c.n_init_good = 50                                    # ... and the configured bound: frame 3 is taken
    post, nids, out, _ = _walk_frame(c, frames, seen, 3, st, ids)
    _check_against_handoff(chain, c, seen, post, nids, out, 3, 5)
    assert nids["landmark_id"][0] == 900 and post["kf_every"] == 3


def test_bounds_eligibility_and_zero_successes():
    st, ids = IR.created()
    xy = np.arange(20, dtype=np.float32).reshape(10, 2)
    ok, X = np.ones(10, bool), np.tile([1.0, 2.0, 30.0], (10, 1))
    tok = np.array([1, 0, 1, 1, 0, 0, 1, 0, 0, 1], bool)
    post, nids, out = IR.init(st, ids, xy, xy - 1, ok, X, tok, 10, 5, 10)               # nRight == init_good is taken; successes == lm_cap fits
    assert out["report"].tolist() == [0, 0, 10, 10, 5, 10, 5, 0] and post["lm"].tolist() == [0, -1, 1, 2, -1, -1, 3, -1, -1, 4]
    assert out["feat_mp_id"].tolist() == [0, -1, 1, 2, -1, -1, 3, -1, -1, 4] and not out["feat_mp_pos"][1].any()
    for args, want in (((10, 4, 10), KR.ERR_CAPACITY), ((9, 5, 10), KR.ERR_CAPACITY), ((10, 5, 11), IR.INIT_RETRY)):
        p, i, o = IR.init(st, ids, xy, xy - 1, ok, X, tok, *args)
        assert o["report"][0] == want and i is ids and o["new_kf_id"] == -1 and o["n_feat"] == 0
        assert (p is st) if want == KR.ERR_CAPACITY else (p["next_frame_id"] == 1)          # capacity keeps the frame id too
    ok2 = ok.copy(); ok2[[0, 2]] = False                    # a success without a right match is not looked at
    assert IR.init(st, ids, xy, xy - 1, ok2, X, tok, 10, 5, 0)[2]["report"].tolist() == [0, 0, 10, 8, 3, 10, 3, 0]
    post, nids, out = IR.init(st, ids, xy, xy - 1, ok, X, np.zeros(10, bool), 10, 5, 0)  # BuildInitMap returns true without a point
    assert out["report"].tolist() == [0, 0, 10, 10, 0, 10, 0, 0] and out["new_kf_id"] == 0 and post["status"] == TR.TRACKING_GOOD and nids["valid"] == 1
    post, nids, out = IR.init(st, ids, xy[:0], xy[:0], ok[:0], X[:0], tok[:0], 10, 5, 0)   # no feature at all, init_good 0
    assert out["report"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0] and nids["next_kf_id"] == 1
    assert IR.init(st, ids, xy[:0], xy[:0], ok[:0], X[:0], tok[:0], 10, 5, 1)[2]["report"][0] == IR.INIT_RETRY
    for kw in ({"frozen": 0}, {"status": TR.TRACKING_GOOD}, {"status": TR.LOST}, {"why": KR.WHY_KEYFRAME}, {"why": KR.WHY_LOST}, {"overflow": 1}):
        s2 = dict(st, **kw)
        p, i, o = IR.init(s2, ids, xy, xy - 1, ok, X, tok, 10, 5, 0)
        assert p is s2 and i is ids and o["report"].tolist() == [KR.NO_TURN, -1, 10, 0, 0, 0, 0, 0] and not IR.mask(4, 6, s2).any()
        assert not (IR.eligible(s2) and KR.eligible(s2, dict(ids, valid=1))), "no stream is eligible for an init and for a turn"
    assert IR.mask(4, 6, st).min() == 255
    with pytest.raises(ValueError):
        IR.reset(st, next_mp_id=-1)


def test_checker_refuses_faulty_devices(pkg):
    """what tests/test_gpu_tracker_init.py would say to a device that ranks off by one, writes a pose that is not the identity, keeps the frame
    id on a retry, or multiplies a non-finite X by the identity"""
    chain = pkg.chain
    st, ids = IR.reset(IR.created()[0], 4, 2, 70, 0)
    xy = np.arange(12, dtype=np.float32).reshape(6, 2)
    ok = np.array([1, 1, 0, 1, 1, 1], bool)
    X = np.array([[1, 2, 30], [0, 0, 0], [0, 0, 0], [3, 1, np.inf], [2, 2, 9], [0, 0, 0]], float)
    tok = np.array([1, 0, 0, 1, 1, 0], bool)
    w = IR.init(st, ids, xy, xy - 2, ok, X, tok, 16, 16, 3)
    good = tuple(IR._copy(d) for d in w)
    IR.check_item("good", good[0], good[1], good[2], *w)

    def refused(fault, needle):
        post, pids, out = (IR._copy(d) for d in w)
        fault(post, pids, out)
        with pytest.raises(AssertionError, match=needle):
            IR.check_item("faulty", post, pids, out, *w)

    def rank_off_by_one(post, pids, out):
        out["feat_mp_id"][out["feat_mp_id"] >= 0] += 1; pids["landmark_id"] += 1
    refused(rank_off_by_one, "feat_mp_id")

    def slot_off_by_one(post, pids, out):
        post["lm"][3], post["lm"][4] = 2, 1
    refused(slot_off_by_one, "state lm")

    def pose_not_identity(post, pids, out):
        out["new_kf_pose"][3] = np.nextafter(1.0, 0.0)
    refused(pose_not_identity, "key-frame pose")

    def ref_pose_not_identity(post, pids, out):
        post["ref_pose"][0] = -0.0                          # the bytes, not the value
    refused(ref_pose_not_identity, "state ref_pose")

    def mv_identity(post, pids, out):                       # mv(I, X) + 0: 0 * inf = NaN in the rows that do not hold the inf
        for arr, rows in ((out["feat_mp_pos"], [0, 3, 4]), (post["lm_pos"], [0, 1, 2])):
            for r in rows:
                arr[r] = chain.mv(np.eye(3), arr[r]) + np.zeros(3)
    with np.errstate(invalid="ignore"):
        refused(mv_identity, "feat_mp_pos")
    assert np.isinf(w[2]["feat_mp_pos"][3, 2]) and not np.isnan(w[2]["feat_mp_pos"]).any(), "the walk keeps X itself"

    r = IR.init(st, ids, xy, xy - 2, ok, X, tok, 16, 16, 6)
    assert r[2]["report"][0] == IR.INIT_RETRY and r[0]["next_frame_id"] == 5
    post, pids, out = (IR._copy(d) for d in r)
    post["next_frame_id"] = 4                                # a device that forgets the constructed Frame
    with pytest.raises(AssertionError, match="state next_frame_id"):
        IR.check_item("faulty", post, pids, out, *r)
    post["next_frame_id"], post["status"] = 5, TR.TRACKING_GOOD
    with pytest.raises(AssertionError, match="state status"):
        IR.check_item("faulty", post, pids, out, *r)
