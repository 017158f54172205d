"""tests/tracker_kf_ref.py (the key-frame turn of the multi-stream tracker walked on plain arrays) is itself checked: beside Chain(OracleBackend)
on the 44-frame stand-in run of tests/test_tracker_ref.py it reproduces, at every key-frame, the detection mask, the feature table after
DetectFeatures, the right start points and tracks of FindFeaturesInRight, the map points of TriangulateNewPoints, the key-frame id and pose of
InsertKeyFrame and the arrays StreamBank.hand_off would upload (taken before the back end optimises and DeepLCD blurs) — the same operators in
the same order, so equality, no tolerance.  The hand-made cases of tests/tracker_kf_cases.py are shown to be made of what their names say.  CPU only."""
import numpy as np

import tracker_cases as TC
import tracker_kf_cases as KC
import tracker_kf_ref as KR
import tracker_ref as TR
from oracle_backend import OracleBackend

CFG = {"numFeatures.trackingGood": 390}
N = 44


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_walk_reproduces_the_chain_at_every_keyframe(pkg, synth, oracle):
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(N)]
    c = chain.Chain(OracleBackend(oracle, synth.calc_weights_handcrafted(), CFG, chain), pkg.api, synth.SEQ_K, frames, cfg=CFG)
    K, base = c.Kt, c.K["baseline"]
    rows, cols = frames[0][0].shape
    seen = {}
    detect, backend = c.be.detect, c.backend_new_keyframe

    def spy_detect(img, mask, init):
        seen["mask"] = mask.copy()
        return detect(img, mask, init)

    def spy_backend(kf):                                  # InsertKeyFrame's frontend half is done; the back end has not run
        seen["handoff"] = TR.state_of_chain(chain, c)
        seen["kf"] = (kf.id, np.array(kf.pose), c.next_kf_id, c.next_mp_id, list(c.outlier_mps))
        seen["right"] = list(c.cur.right)
        seen["feat_ids"] = [(f.mp.id if f.live() is not None else -1) for f in kf.feats]
        return backend(kf)

    c.be.detect, c.backend_new_keyframe = spy_detect, spy_backend
    assert c.grab(0) and c.status == chain.TRACKING_GOOD
    st, lids = TR.state_of_chain(chain, c)
    n_kf = n_new_mp = n_dropped = 0
    for t in range(1, N):
        prev = c.last.L
        n_log, n_out = len(c.log), len(c.outlier_mps)
        ids = {"landmark_id": np.array(lids, np.int64), "ref_kf_id": c.ref_kf.id, "next_kf_id": c.next_kf_id, "next_mp_id": c.next_mp_id, "valid": 1}
        new, rec, _ = TR.step(chain, oracle, K, st, prev, frames[t][0], c.n_good, c.n_bad)
        assert c.grab(t)
        if not rec["needs_host"]:
            st = new
            continue
        tag = f"frame {t}"
        log = {k: v for k, v in c.log[n_log:]}
        pre = dict(new, why=KR.why_of(rec))
        assert pre["why"] == KR.WHY_KEYFRAME and KR.eligible(pre, ids)
        # DetectFeatures: mask and table
        assert _same(seen["mask"], KR.mask(rows, cols, pre, ids)), tag + ": mask"
        kps = log["detect"][0]
        new_xy = np.stack([kps["x"], kps["y"]], 1).astype(np.float32)
        p0, p1, lm = KR.append_and_starts(chain, K, base, pre, new_xy)
        # FindFeaturesInRight
        nxt, ok, lp1 = log["lk_right"]
        assert _same(lp1, p1), tag + ": right start points"
        ok = np.asarray(ok, bool)
        assert [(r is not None) for r in seen["right"]] == ok.tolist()
        # TriangulateNewPoints: the chain's accepted triangulation, spread over the candidates
        cand = KR.candidates(lm, ok)
        xyz, tok = np.zeros((len(p0), 3)), np.zeros(len(p0), bool)
        if cand:
            tok[cand] = np.asarray(log["triangulate"][0], bool)
            xyz[[i for i in cand if tok[i]]] = log["triangulate"][1]
        post, nids, out = KR.turn(chain, K, base, pre, ids, new_xy, nxt, ok, xyz, tok, 4096, 8192)
        want, wids = seen["handoff"]
        kf_id, kf_pose, next_kf, next_mp, outl = seen["kf"]
        assert out["report"][0] == 0 and out["new_kf_id"] == kf_id and _same(out["new_kf_pose"], kf_pose), tag + ": key-frame id / pose"
        assert (nids["ref_kf_id"], nids["next_kf_id"], nids["next_mp_id"]) == (kf_id, next_kf, next_mp), tag + ": id counters"
        assert out["outlier_mp_id"].tolist() == outl[len(outl) - out["n_outlier_mp"]:] and out["n_outlier_mp"] == len(pre["outlier_list"]), tag + ": outlier ids"
        feats = c.all_kfs[kf_id].feats
        assert seen["feat_ids"] == out["feat_mp_id"].tolist(), tag + ": map-point ids by feature"
        assert _same(np.array([[f.x, f.y] for f in feats], np.float32), out["feat_uv"]) and out["n_feat"] == len(feats)
        for k in ("xy", "lm", "lm_pos", "lm_outlier", "ref_pose", "last_rel", "rel_motion"):      # (lm_pos: the positions before the back end moves them)
            assert np.asarray(want[k]).dtype == np.asarray(post[k]).dtype and _same(want[k], post[k]), tag + ": hand-off " + k
        assert all(_same(post["lm_pos"][post["lm"][i]], out["feat_mp_pos"][i]) for i in range(len(feats)) if post["lm"][i] >= 0)
        assert (want["ref_frame_id"], want["next_frame_id"], want["status"]) == (post["ref_frame_id"], post["next_frame_id"], post["status"]), tag
        assert nids["landmark_id"].tolist() == wids, tag + ": landmark ids by slot"
        assert post["frozen"] == 0 and len(post["outlier_list"]) == 0
        n_kf += 1; n_new_mp += int(out["report"][4]); n_dropped += int(len(pre["lm_pos"]) + out["report"][4] - out["report"][6])
        st, lids = TR.state_of_chain(chain, c)            # after the back end (BA, blur): the chain's next hand-off
    assert n_kf >= 7 and n_new_mp > 100 and n_dropped > 0, (n_kf, n_new_mp, n_dropped)


class _Ops:
    """the oracle's operators under the names tracker_kf_ref.turn_with uses"""
    def __init__(self, oracle):
        self.lk_track, self.triangulate_stereo = oracle.lk_track, oracle.triangulate_stereo


def _walk(chain, oracle, case, cap=1024, lm_cap=2048, **kw):
    st = dict(case["st"], frozen=1, why=KR.WHY_KEYFRAME, outlier_list=np.zeros(0, np.int32))
    st.update(kw)
    ids = dict(case["ids"], valid=1)
    return (st, ids) + KR.turn_with(chain, _Ops(oracle), case["K"], KC.BASELINE, st, ids, case["left"], case["right"], case["new_xy"], cap, lm_cap)


def test_rich_case_is_made_of_what_it_says(pkg, synth, oracle):
    chain = pkg.chain
    case = KC.rich_case(chain, synth)
    st, ids, post, nids, out, dbg = _walk(chain, oracle, case)
    n = len(st["lm"])
    assert out["report"][0] == 0
    assert st["lm"][13] == st["lm"][14] == -1 and dbg["tri_ok"][13] and dbg["tri_ok"][14], "kept features without a landmark triangulate mid-table"
    assert 0 < post["lm"][12] < post["lm"][13] < post["lm"][14] < post["lm"][15], "their slots lie between their neighbours' (first-reference order)"
    assert st["lm_outlier"][st["lm"][5]] == 1 and st["lm"][20] == st["lm"][5] and _same(dbg["p1"][5], dbg["p0"][5]), "flagged landmark: own pixel"
    assert post["lm"][5] == post["lm"][20] and post["lm_outlier"][post["lm"][5]] == 1 and nids["landmark_id"][post["lm"][5]] == ids["landmark_id"][5]
    assert st["lm"][1] == st["lm"][2] and post["lm"][1] == post["lm"][2]
    assert not dbg["right_ok"][30] and not dbg["right_ok"][31] and dbg["p1"][30][0] < -100, "right tracks lost outside the image"
    assert len(post["lm_pos"]) == out["report"][6] < len(st["lm_pos"]) + out["report"][4], "unreferenced landmarks are dropped"
    assert out["report"][4] >= 10 and np.all(out["feat_mp_id"][n:][dbg["tri_ok"][n:]] >= ids["next_mp_id"])
    # order by old slot would differ: slot 13's and 14's landmarks are gone, new points sit between old ones
    old_order = [l for l in range(len(st["lm_pos"])) if l in set(st["lm"].tolist())]
    assert nids["landmark_id"][:len(old_order)].tolist() != ids["landmark_id"][old_order].tolist()
    # plain features: the start point is the landmark seen from the right camera, 3 px left of the feature
    plain = [i for i in range(n) if st["lm"][i] >= 0 and not st["lm_outlier"][st["lm"][i]] and i not in case["near"]]
    assert np.abs(dbg["p1"][plain] - (dbg["p0"][plain] - np.float32([3, 0]))).max() < 1e-3
    assert np.abs(dbg["right_xy"][plain][dbg["right_ok"][plain]] - (dbg["p0"][plain][dbg["right_ok"][plain]] - np.float32([3, 0]))).max() < 0.1


def test_disparity_counts_sizes_and_se3_cases(pkg, synth, oracle):
    chain = pkg.chain
    for case in KC.disparity_cases(chain, synth):
        st, ids, post, nids, out, dbg = _walk(chain, oracle, case)
        n = len(st["lm"])
        assert out["report"][0] == 0 and dbg["right_ok"][n:].sum() >= 12, case["name"]
        if case["d"] < 0:                                # behind the cameras: z > 0 fails for every candidate
            assert out["report"][4] == 0 and nids["next_mp_id"] == ids["next_mp_id"] and np.all(post["lm"][n:] == -1), case["name"]
        else:                                            # disparity 0: points at infinity, the solve divides by (nearly) zero; whatever it gives, z is not finite-positive-small
            assert not np.any(dbg["tri_ok"] & (np.abs(dbg["tri_xyz"][:, 2]) < 1e3)), case["name"]
    for total in KC.TOTALS:
        case = KC.total_case(chain, synth, total)
        assert len(case["st"]["lm"]) + len(case["new_xy"]) == total
        out = _walk(chain, oracle, case)[4]
        assert out["report"][0] == 0 and out["report"][5] == total
    over = KC.total_case(chain, synth, 1025)
    st, ids, post, nids, out, _ = _walk(chain, oracle, over)
    assert out["report"][0] == KR.ERR_CAPACITY and post is st and nids is ids and out["new_kf_id"] == -1 and out["n_feat"] == 0
    rich = KC.rich_case(chain, synth)
    full = _walk(chain, oracle, rich)[4]["report"][6]
    assert _walk(chain, oracle, rich, lm_cap=full)[4]["report"][0] == 0 and _walk(chain, oracle, rich, lm_cap=full - 1)[4]["report"][0] == KR.ERR_CAPACITY
    branches = set()
    for case in KC.se3_cases(chain, synth):
        st, ids, post, nids, out, dbg = _walk(chain, oracle, case)
        Tcw = KR.Tcw_of(chain, st)
        branches.add(TC.branch_of(Tcw[:3, :3])); branches.add(TC.branch_of(chain.T_inv(Tcw)[:3, :3]))
        assert out["report"][0] == 0 and _same(post["ref_pose"], chain.p7_of(Tcw)) and _same(post["last_rel"], np.eye(4))
    assert {b for b, _ in branches} == {0, 1, 2, 3} and any(f for _, f in branches)
    for case in KC.size_cases(chain, synth):
        assert _walk(chain, oracle, case)[4]["report"][4] >= 10, case["name"]
    # not eligible: LOST, capacity, never recorded, ids not valid
    for kw, valid in (({"why": KR.WHY_LOST}, 1), ({"why": KR.WHY_CAPACITY}, 1), ({"why": KR.WHY_NONE}, 1), ({"frozen": 0}, 1), ({}, 0)):
        st = dict(rich["st"], frozen=1, why=KR.WHY_KEYFRAME, outlier_list=np.zeros(0, np.int32)); st.update(kw)
        ids = dict(rich["ids"], valid=valid)
        post, nids, out = KR.turn(chain, rich["K"], KC.BASELINE, st, ids, rich["new_xy"], None, None, None, None, 1024, 2048)
        assert post is st and nids is ids and out["report"][0] == KR.NO_TURN and out["new_kf_id"] == -1
        assert not KR.mask(120, 160, st, ids).any()


class _MaskSpy:
    def detect(self, img, mask, init):
        self.mask = mask.copy()
        return np.zeros(0, dtype=[("x", "<f4"), ("y", "<f4")])


def test_mask_is_the_chains_mask(pkg):
    chain = pkg.chain
    rows, cols = 120, 160
    tabs = KC.mask_tables(rows, cols, 300)
    for name, xy in tabs.items():
        st = dict(KC.table_state(chain, xy), frozen=1, why=KR.WHY_KEYFRAME)
        got = KR.mask(rows, cols, st, {"valid": 1})
        if name == "nonfinite":                       # the chain cannot round a NaN: the walk draws the finite feature alone
            st2 = dict(KC.table_state(chain, xy[3:]), frozen=1, why=KR.WHY_KEYFRAME)
            assert _same(got, KR.mask(rows, cols, st2, {"valid": 1})) and got[80, 100] == 0 and got.min() == 0 and got[10, 10] == 255
            continue
        spy = _MaskSpy()
        c = chain.Chain(spy, pkg.api, {"fx": 1.0, "fy": 1.0, "cx": 0.0, "cy": 0.0, "bf": 1.0}, [], log=False)
        c.cur = chain.Frame(0, 0.0, np.zeros((rows, cols), np.uint8), None)
        c.cur.feats = [chain.Feature(x, y) for x, y in xy]
        c.status = chain.TRACKING_GOOD
        c.detect_features()
        assert _same(spy.mask, got), name
    assert KR.mask(rows, cols, dict(KC.table_state(chain, tabs["outside"]), frozen=1, why=KR.WHY_KEYFRAME), {"valid": 1}).min() == 255
    half = KR.mask(rows, cols, dict(KC.table_state(chain, tabs["half"][:2]), frozen=1, why=KR.WHY_KEYFRAME), {"valid": 1})
    # (50.5, 40.5): columns rint(30.5) = 30 .. rint(70.5) = 70, rows 20 .. 60; (51.5, 41.5): columns rint(31.5) = 32 .. rint(71.5) = 72, rows 22 .. 62
    # (ties to even; half up would give 31 .. 71 and 32 .. 72).  Row 20 lies in the first rectangle only, row 62 in the second only.
    assert half[20, 29] == 255 and half[20, 30] == 0 and half[20, 70] == 0 and half[20, 71] == 255 and half[19, 50] == 255
    assert half[62, 31] == 255 and half[62, 32] == 0 and half[62, 72] == 0 and half[62, 73] == 255 and half[63, 50] == 255
    assert KR.cv_round(np.float32(0.5)) == 0 and KR.cv_round(np.float32(1.5)) == 2 and KR.cv_round(np.float32(-0.5)) == 0 and KR.cv_round(np.float32(2.5)) == 2
