"""StereoInit on the device composed with what follows it on the GPU.
Composition: chain.StreamBank over 3 rendered streams whose streams START on the device (masks -> detect_batch on the init extractor ->
init_batch) and take their key-frame turns there, against the same bank on the host paths (Chain.grab + hand_off, host_turn), the back end's
optimisation and DeepLCD's blur switched off on both sides: states, ids, stored images and result records are equal byte for byte at every
step, through at least two turns per stream.  (get_frame downloads a stored image only for a stream that was given one through set_frame: the
device bank's streams are given a black one and reset before the first frame.)
Chain, from nothing: init_batch -> myslam_backend_insert_keyframe_batch on EMPTY tables -> step -> turn -> insert -> myslam_backend_optimize_batch
-> update_from_map -> step, with status 0 throughout and not one host-pointer call between create and the last step."""
import numpy as np
import pytest

from test_gpu_tracker_kf import STATE_KEYS, _same, _state_bytes
from test_gpu_tracker_kf_chain import KF_EVERY, OFFSETS, _bank

pytestmark = pytest.mark.gpu

STEPS = 12


def test_device_init_equals_host_init_step_by_step(api, pkg, synth):
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(max(OFFSETS) + STEPS + 2)]
    dev, host = _bank(pkg, api, synth, frames, True), _bank(pkg, api, synth, frames, False)
    dev.device_init, dev.resync_init = True, False
    assert host.device_init is False
    rows, cols = frames[0][0].shape
    for s in range(3):                                   # an image mark for get_frame(image=True); the bank arms (resets) the streams itself
        dev.trk.set_frame(s, dict(dev.trk.get_frame(s), status=0), image=np.zeros((rows, cols), np.uint8))
        dev.trk.reset_stream(s)
    for t in range(STEPS + 1):
        a, b = dev.advance(t), host.advance(t)
        assert a == b == [0, 1, 2]
        if t:
            assert dev.results().tobytes() == host.results().tobytes(), f"step {t}: result records"
        for s in range(3):
            sa, sb = (dev.trk.get_frame(s, image=True), dev.trk.get_ids(s)), (host.trk.get_frame(s, image=True), host.trk.get_ids(s))
            for k, x, y in zip(list(STATE_KEYS) + sorted(sa[1]), _state_bytes(*sa), _state_bytes(*sb)):
                assert x == y, f"step {t} stream {s}: {k}"
        if t == 0:
            assert all(c.status == pkg.chain.TRACKING_GOOD and c.kf_frames == [0] and len(c.all_mps) > 50 for c in dev.chains)
            assert dev.trk.get_frame(0)["kf_every"] == KF_EVERY[0] and dev.on_device == [True] * 3
    turns = [len(c.kf_frames) - 1 for c in dev.chains]
    assert min(turns) >= 2 and [c.kf_frames for c in dev.chains] == [c.kf_frames for c in host.chains], turns
    for ca, cb in zip(dev.chains, host.chains):          # the chains' maps hold the same key-frames and map points, and the same trajectory
        assert sorted(ca.all_kfs) == sorted(cb.all_kfs) and sorted(ca.all_mps) == sorted(cb.all_mps)
        assert all(_same(ca.all_kfs[i].pose, cb.all_kfs[i].pose) for i in ca.all_kfs) and all(_same(ca.all_mps[i].pos, cb.all_mps[i].pos) for i in ca.all_mps)
        assert (ca.next_frame_id, ca.next_kf_id, ca.next_mp_id, ca.outlier_mps) == (cb.next_frame_id, cb.next_kf_id, cb.next_mp_id, cb.outlier_mps)
        assert len(ca.poses) == len(cb.poses) and all(_same(np.asarray(p, float), np.asarray(q, float)) for p, q in zip(ca.poses, cb.poses))
        assert [len(f.mp.obs) if f.live() is not None else -1 for f in ca.all_kfs[0].feats] == [len(f.mp.obs) if f.live() is not None else -1 for f in cb.all_kfs[0].feats]
    print(f"composition: device init + {turns} device turns per stream over {STEPS} steps, {dev.trk.init_launches()} launches per init")


def test_retry_on_the_device_spends_a_frame_like_the_host(api, pkg, synth):
    """numFeatures.initGood above the match count for two frames: both banks drop them, then both start on frame 2 as key-frame 0"""
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(max(OFFSETS) + 5)]
    dev, host = _bank(pkg, api, synth, frames, True), _bank(pkg, api, synth, frames, False)
    dev.device_init, dev.resync_init = True, False
    for t in range(4):
        for bank in (dev, host):
            for c in bank.chains:
                c.n_init_good = 100000 if t < 2 else 50
        assert dev.advance(t) == host.advance(t) == [0, 1, 2]
        for s in range(3):
            ca, cb = dev.chains[s], host.chains[s]
            assert (ca.status, ca.next_frame_id, ca.next_kf_id, ca.kf_frames) == (cb.status, cb.next_frame_id, cb.next_kf_id, cb.kf_frames), (t, s)
            assert ca.status == (pkg.chain.INITING if t < 2 else pkg.chain.TRACKING_GOOD) and len(ca.poses) == len(cb.poses) == t + 1
            sa, sb = (dev.trk.get_frame(s), dev.trk.get_ids(s)), (host.trk.get_frame(s), host.trk.get_ids(s))
            if t >= 2:
                for k in [k for k in STATE_KEYS if k != "image"]:
                    assert _same(sa[0][k], sb[0][k]), f"frame {t} stream {s}: {k}"
                assert all(_same(sa[1][k], sb[1][k]) for k in sa[1]) and sa[0]["ref_frame_id"] == 2 and sa[1]["ref_kf_id"] == 0
            else:
                assert sa[0]["next_frame_id"] == t + 1 and sa[0]["frozen"] == 1 and sa[0]["status"] == 0 and len(sa[0]["xy"]) == 0
    assert dev.results().tobytes() == host.results().tobytes()


def test_from_nothing_init_insert_step_turn_insert_optimise_update_step(api, pkg, synth):
    import torch
    chain = pkg.chain
    S, KFC, MPC, OBC, WINDOW, CAP = 3, 8, 1024, 4096, 7, 1024
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [[synth.render_stereo(scene, C[o + t], yaw[o + t], o + t) for o in OFFSETS] for t in range(2)]
    rows, cols = frames[0][0][0].shape
    img = rows * cols
    K = synth.SEQ_K
    Kt, base = (K["fx"], K["fy"], K["cx"], K["cy"]), K["bf"] / K["fx"]
    hb = chain.HipBackend(api, lcd=api.DeepLCD(synth.calc_weights_handcrafted()))
    trk = api.Tracker(S, rows, cols, CAP, 2048, Kt, 20, -1)              # tracking_bad -1: never LOST; the turn is forced below
    be = api.Backend(S, KFC, MPC, OBC)
    z = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device="cuda")
    T = {"kf_id": z((S, KFC), "int64"), "kf_pose": z((S, KFC, 7), "float64"), "n_kf": z((S,), "int32"), "mp_id": z((S, MPC), "int64"),
         "mp_pos": z((S, MPC, 3), "float64"), "mp_outlier": z((S, MPC), "uint8"), "n_mp": z((S,), "int32"), "obs_mp": z((S, OBC), "int32"),
         "obs_kf": z((S, OBC), "int32"), "obs_flags": z((S, OBC), "uint8"), "obs_uv": z((S, OBC, 2), "float32"), "obs_tag": z((S, OBC), "int32"),
         "n_obs": z((S,), "int32")}
    order = ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")
    I = {"feat_row": z((S, CAP), "int32"), "mp_new_row": z((S, MPC), "int32"), "removed_kf_id": z((S,), "int64"), "removed_kf_row": z((S,), "int32"),
         "dis": z((S, KFC), "float64"), "status": z((S,), "int32")}
    O = {"obs_report": z((S, OBC), "uint8"), "mp_report": z((S, MPC), "uint8"), "new_outlier": z((S, MPC), "int32"), "n_new": z((S,), "int32"),
         "obs_chi2": z((S, OBC), "float64"), "rounds": z((S,), "int32"), "n_out": z((S,), "int32"), "status": z((S,), "int32")}
    out = {"new_kf_id": z(S, "int64"), "new_kf_pose": z((S, 7), "float64"), "feat_mp_id": z((S, CAP), "int64"), "feat_mp_pos": z((S, CAP, 3), "float64"),
           "feat_uv": z((S, CAP, 2), "float32"), "feat_tag": z((S, CAP), "int32"), "feat_flags": z((S, CAP), "uint8"), "n_feat": z(S, "int32"),
           "outlier_mp_id": z((S, 2 * CAP), "int64"), "n_outlier_mp": z(S, "int32"), "right_xy": z((S, CAP, 2), "float32"), "right_ok": z((S, CAP), "uint8"),
           "report": z((S, 8), "int32")}
    optr = {k: v.data_ptr() for k, v in out.items()}
    kp_cap = max(int(hb.det_init.max_keypoints(rows, cols)), int(hb.orb.max_keypoints(rows, cols)))
    d_kps, d_nkp, d_kst = z((S, kp_cap, api.KP_DTYPE.itemsize), "uint8"), z(S, "int32"), z(S, "int32")
    d_mask, d_res = z((S, rows, cols), "uint8"), z(S * 80, "uint8")
    d_L = [torch.from_numpy(np.stack([np.ascontiguousarray(L) for L, _ in fr])).cuda() for fr in frames]
    d_R = [torch.from_numpy(np.stack([np.ascontiguousarray(R) for _, R in fr])).cuda() for fr in frames]

    def insert():
        be.insert_keyframe_batch(*[T[k].data_ptr() for k in order], *[optr[k] for k in ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos", "feat_uv",
                                 "feat_tag", "feat_flags", "n_feat")], CAP, 0, 0, 0, 0, 0, 0, 1, optr["outlier_mp_id"], optr["n_outlier_mp"], 2 * CAP, S, WINDOW,
                                 0.2, *[I[k].data_ptr() for k in ("feat_row", "mp_new_row", "removed_kf_id", "removed_kf_row", "dis", "status")])

    # ---- from nothing: a created tracker, empty tables ----
    trk.init_masks(d_mask.data_ptr(), cols, img)
    hb.det_init.detect_batch(d_L[0].data_ptr(), S, rows, cols, cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), d_kst.data_ptr(), kp_cap, d_masks=d_mask.data_ptr())
    trk.init_batch(d_L[0].data_ptr(), d_R[0].data_ptr(), cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), kp_cap, base, 50, optr)
    insert()
    trk.step_batch(d_L[1].data_ptr(), cols, img, d_res.data_ptr())
    torch.cuda.synchronize()
    rep = out["report"].cpu().numpy()
    assert rep[:, 0].tolist() == [0, 0, 0] and (rep[:, 4] > 50).all() and out["new_kf_id"].cpu().numpy().tolist() == [0, 0, 0], rep
    assert I["status"].cpu().numpy().tolist() == [0, 0, 0] and T["n_kf"].cpu().numpy().tolist() == [1, 1, 1]
    n_mp = T["n_mp"].cpu().numpy()
    assert n_mp.tolist() == rep[:, 4].tolist(), "every success is a map-point row"
    for s in range(S):
        assert T["mp_id"].cpu().numpy()[s, :n_mp[s]].tolist() == list(range(n_mp[s])) and _same(T["kf_pose"].cpu().numpy()[s, 0], chain.IDENT)
        assert T["n_obs"].cpu().numpy()[s] == n_mp[s]
    res = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE).copy()
    assert (res["status"] == chain.TRACKING_GOOD).all() and res["frame_id"].tolist() == [1, 1, 1] and (res["n_inliers"] > 50).all(), res
    assert (res["needs_host"] == 0).all()
    # ---- the key-frame rule fires (forced: the test seam), the turn, the second key-frame, the optimisation, the way back, the next step ----
    for s in range(S):
        trk.debug_freeze(s, 1)
    trk.keyframe_masks(d_mask.data_ptr(), cols, img)
    hb.orb.detect_batch(d_L[1].data_ptr(), S, rows, cols, cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), d_kst.data_ptr(), kp_cap, d_masks=d_mask.data_ptr())
    trk.keyframe_batch(d_R[1].data_ptr(), cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), kp_cap, base, optr)
    insert()
    be.optimize_batch(*[T[k].data_ptr() for k in order], S, Kt, *[O[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2",
                      "rounds", "n_out", "status")])
    trk.update_from_map(T["kf_id"].data_ptr(), T["kf_pose"].data_ptr(), T["n_kf"].data_ptr(), KFC, T["mp_id"].data_ptr(), T["mp_pos"].data_ptr(),
                        T["mp_outlier"].data_ptr(), T["n_mp"].data_ptr(), MPC)
    trk.step_batch(d_L[1].data_ptr(), cols, img, d_res.data_ptr())
    torch.cuda.synchronize()
    rep2 = out["report"].cpu().numpy()
    assert rep2[:, 0].tolist() == [0, 0, 0] and out["new_kf_id"].cpu().numpy().tolist() == [1, 1, 1], rep2
    assert I["status"].cpu().numpy().tolist() == [0, 0, 0] and O["status"].cpu().numpy().tolist() == [0, 0, 0] and T["n_kf"].cpu().numpy().tolist() == [2, 2, 2]
    assert (T["n_mp"].cpu().numpy() == n_mp + rep2[:, 4]).all()
    res2 = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert (res2["status"] == chain.TRACKING_GOOD).all() and res2["frame_id"].tolist() == [2, 2, 2] and (res2["n_inliers"] > 50).all(), res2
    tab = {k: v.cpu().numpy() for k, v in T.items()}
    for s in range(S):                                   # the tracker's landmarks and reference pose are the tables' rows
        st, ids = trk.get_frame(s), trk.get_ids(s)
        row = {int(i): r for r, i in enumerate(tab["mp_id"][s, :tab["n_mp"][s]])}
        held = [l for l, i in enumerate(ids["landmark_id"]) if int(i) in row]
        assert len(held) >= len(ids["landmark_id"]) // 2 and all(_same(st["lm_pos"][l], tab["mp_pos"][s, row[int(ids["landmark_id"][l])]]) for l in held)
        assert ids["ref_kf_id"] == 1 and _same(st["ref_pose"], tab["kf_pose"][s, list(tab["kf_id"][s, :2]).index(1)])
