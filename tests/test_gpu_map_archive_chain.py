"""The map archive inside the from-nothing composition of tests/test_gpu_tracker_init_chain.py, 3 rendered streams:
init_batch -> insert (EMPTY tables) -> map update -> step -> turn -> insert -> map update -> optimise -> map update -> update_from_map -> step.  After every map update the archive of every stream (read back there) must equal tests/map_archive_ref.py's walk fed the
tables, statuses, outlier ids and reports the device left at that stage; then the feature slots of the turn's features are a search of the archive."""
import numpy as np
import pytest

import map_archive_ref as mr
from test_gpu_map_archive import tables_of
from test_gpu_tracker_kf_chain import OFFSETS

pytestmark = pytest.mark.gpu


def test_from_nothing_with_the_archive_at_every_stage(api, pkg, synth):
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
    arc = api.MapArchive(S, 16, 15, 2048, MPC)
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
    walks = [mr.Archive() for _ in range(S)]
    d_slots = z((S, CAP), "int32")

    def insert():
        be.insert_keyframe_batch(*[T[k].data_ptr() for k in order], *[optr[k] for k in ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos", "feat_uv",
                                 "feat_tag", "feat_flags", "n_feat")], CAP, 0, 0, 0, 0, 0, 0, 1, optr["outlier_mp_id"], optr["n_outlier_mp"], 2 * CAP, S, WINDOW,
                                 0.2, *[I[k].data_ptr() for k in ("feat_row", "mp_new_row", "removed_kf_id", "removed_kf_row", "dis", "status")])

    def update(mode, stage):
        """the map update of this stage, then (the test reads back here; the calls themselves never synchronise) the walk fed the downloaded tables"""
        st = z(S, "int32") - 9
        be_st = I["status"] if mode == mr.AFTER_INSERT else O["status"]
        arc.update_batch(mode, T["kf_id"].data_ptr(), T["kf_pose"].data_ptr(), T["n_kf"].data_ptr(), KFC, T["mp_id"].data_ptr(), T["mp_pos"].data_ptr(),
                         T["n_mp"].data_ptr(), MPC, T["obs_mp"].data_ptr(), T["obs_kf"].data_ptr(), T["obs_flags"].data_ptr(), T["n_obs"].data_ptr(), OBC,
                         be_st.data_ptr(), optr["outlier_mp_id"], optr["n_outlier_mp"], 2 * CAP, O["mp_report"].data_ptr(), S, st.data_ptr())
        torch.cuda.synchronize()
        host = {k: T[k].cpu().numpy() for k in order}
        outl, n_outl, rep = out["outlier_mp_id"].cpu().numpy(), out["n_outlier_mp"].cpu().numpy(), O["mp_report"].cpu().numpy()
        assert be_st.cpu().numpy().tolist() == [0, 0, 0], stage
        for s, a in enumerate(walks):
            want = mr.update(chain, a, mode, tables_of(host, s), 0, outlier_ids=outl[s, :n_outl[s]], mp_report=rep[s], caps=(16, 15, 2048))
            assert int(st[s]) == want == mr.UPDATED, (stage, s, int(st[s]), want)
            assert mr.same(arc.get(s), a.arrays()) is None, (stage, s, mr.same(arc.get(s), a.arrays()))

    # ---- from nothing: a created tracker, empty tables, an empty archive ----
    trk.init_masks(d_mask.data_ptr(), cols, img)
    hb.det_init.detect_batch(d_L[0].data_ptr(), S, rows, cols, cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), d_kst.data_ptr(), kp_cap, d_masks=d_mask.data_ptr())
    trk.init_batch(d_L[0].data_ptr(), d_R[0].data_ptr(), cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), kp_cap, base, 50, optr)
    insert()
    update(mr.AFTER_INSERT, "init")
    trk.step_batch(d_L[1].data_ptr(), cols, img, d_res.data_ptr())
    for s in range(S):
        trk.debug_freeze(s, 1)
    trk.keyframe_masks(d_mask.data_ptr(), cols, img)
    hb.orb.detect_batch(d_L[1].data_ptr(), S, rows, cols, cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), d_kst.data_ptr(), kp_cap, d_masks=d_mask.data_ptr())
    trk.keyframe_batch(d_R[1].data_ptr(), cols, img, d_kps.data_ptr(), d_nkp.data_ptr(), kp_cap, base, optr)
    insert()
    update(mr.AFTER_INSERT, "turn")
    be.optimize_batch(*[T[k].data_ptr() for k in order], S, Kt, *[O[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2",
                      "rounds", "n_out", "status")])
    update(mr.AFTER_OPTIMIZE, "optimise")
    arc.feature_slots_batch(optr["feat_mp_id"], optr["n_feat"], CAP, S, d_slots.data_ptr())
    # the corrector's index inputs for "key-frame 1 closes a loop with key-frame 0" (the archive holds more points than one block of k_map_loop_inputs takes)
    L = {"active": z((S, 10), "int32") - 5, "n_active": z(S, "int32"), "cur": z(S, "int32"), "loop": z(S, "int32"), "first_active": z((S, 2048), "int32") - 5,
         "first_kf": z((S, 2048), "int32") - 5, "n_points": z(S, "int32")}
    d_loop_id, d_det = z(S, "int64"), z(S, "int32")
    arc.loop_inputs_batch(T["kf_id"].data_ptr(), T["n_kf"].data_ptr(), KFC, T["mp_id"].data_ptr(), T["n_mp"].data_ptr(), MPC, T["obs_mp"].data_ptr(),
                          T["obs_kf"].data_ptr(), T["obs_flags"].data_ptr(), T["n_obs"].data_ptr(), OBC, optr["new_kf_id"], d_loop_id.data_ptr(), d_det.data_ptr(), 10, S,
                          *[L[k].data_ptr() for k in ("active", "n_active", "cur", "loop", "first_active", "first_kf", "n_points")])
    trk.update_from_map(T["kf_id"].data_ptr(), T["kf_pose"].data_ptr(), T["n_kf"].data_ptr(), KFC, T["mp_id"].data_ptr(), T["mp_pos"].data_ptr(),
                        T["mp_outlier"].data_ptr(), T["n_mp"].data_ptr(), MPC)
    trk.step_batch(d_L[1].data_ptr(), cols, img, d_res.data_ptr())
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert (res["status"] == chain.TRACKING_GOOD).all() and res["frame_id"].tolist() == [2, 2, 2]
    host = {k: T[k].cpu().numpy() for k in order}
    Lh = {k: v.cpu().numpy() for k, v in L.items()}
    for s, a in enumerate(walks):
        want = mr.loop_inputs(a, tables_of(host, s), 1, 0, 0)
        n = want["n_points"]
        assert n > 256 and Lh["n_points"][s] == n and Lh["n_active"][s] == 2 and Lh["active"][s].tolist() == [0, 1] + [-5] * 8
        assert (Lh["cur"][s], Lh["loop"][s]) == (want["cur"], want["loop"]) == (1, 0)
        assert np.array_equal(Lh["first_active"][s, :n], want["first_active"]) and np.array_equal(Lh["first_kf"][s, :n], want["first_kf"])
        assert (Lh["first_active"][s, n:] == -5).all() and (Lh["first_kf"][s, n:] == -5).all() and (want["first_active"] >= 0).sum() > 100
        assert a.kf_id == [0, 1] and a.edge_v0 == [1] and a.edge_v1 == [0] and len(a.mp_id) > 100
        nf = int(out["n_feat"].cpu().numpy()[s])
        assert np.array_equal(d_slots.cpu().numpy()[s, :nf], mr.feature_slots(a, out["feat_mp_id"].cpu().numpy()[s, :nf]))
