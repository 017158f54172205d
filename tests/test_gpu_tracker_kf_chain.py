"""The key-frame turn composed with what stands before and after it on the GPU.
Composition: chain.StreamBank over 3 rendered streams whose frozen streams take their turn ON THE DEVICE (step -> masks -> detect_batch -> turn ->
step) against the same bank taking StreamBank.host_turn (get_frame, the three single-image calls, set_frame), the back end's optimisation and
DeepLCD's blur switched off on both sides: states, ids, stored images and result records are equal byte for byte at every step.
Chain: turn -> myslam_backend_insert_keyframe_batch -> myslam_backend_optimize_batch -> update_from_map -> step with status 0 throughout, and the
tracker's landmarks are the table's rows afterwards; what the insert call does with a no-turn item is what the header says."""
import numpy as np
import pytest

import tracker_kf_cases as KC
import tracker_kf_ref as KR
from test_gpu_tracker_kf import Rig, STATE_KEYS, _same, _state_bytes

pytestmark = pytest.mark.gpu

OFFSETS, KF_EVERY, STEPS = [0, 3, 7], [4, 4, 5], 22


def _bank(pkg, api, synth, frames, device):
    chain = pkg.chain
    lcd = api.DeepLCD(synth.calc_weights_handcrafted())
    mk = lambda o: (lambda t: frames[o + t])
    chains = [chain.Chain(chain.HipBackend(api, lcd=lcd), api, synth.SEQ_K, mk(o), kf_every=k, log=False) for o, k in zip(OFFSETS, KF_EVERY)]
    for c in chains:                                     # the map keeps its books, but moves no point, kills none and blurs no image
        c.optimize_active_map = lambda: None
        c.lc_insert_new_keyframe = lambda kf: False
    bank = chain.StreamBank(chains, api, cap=1024, landmark_cap=2048)
    bank.device_turns, bank.resync_turns = device, False
    return bank


def test_device_turns_equal_host_turns_step_by_step(api, pkg, synth):
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(max(OFFSETS) + STEPS + 2)]
    dev, host = _bank(pkg, api, synth, frames, True), _bank(pkg, api, synth, frames, False)
    for t in range(STEPS + 1):
        a, b = dev.advance(t), host.advance(t)
        assert a == b == [0, 1, 2]
        if t:
            assert dev.results().tobytes() == host.results().tobytes(), f"step {t}: result records"
        for s in range(3):
            sa, sb = (dev.trk.get_frame(s, image=True), dev.trk.get_ids(s)), (host.trk.get_frame(s, image=True), host.trk.get_ids(s))
            for k, x, y in zip(list(STATE_KEYS) + sorted(sa[1]), _state_bytes(*sa), _state_bytes(*sb)):
                assert x == y, f"step {t} stream {s}: {k}"
    turns = [len(c.kf_frames) - 1 for c in dev.chains]
    assert min(turns) >= 4 and [c.kf_frames for c in dev.chains] == [c.kf_frames for c in host.chains], turns
    for ca, cb in zip(dev.chains, host.chains):          # the chains' maps hold the same key-frames and map points
        assert sorted(ca.all_kfs) == sorted(cb.all_kfs) and sorted(ca.all_mps) == sorted(cb.all_mps)
        assert all(_same(ca.all_kfs[i].pose, cb.all_kfs[i].pose) for i in ca.all_kfs) and all(_same(ca.all_mps[i].pos, cb.all_mps[i].pos) for i in ca.all_mps)
        assert (ca.next_kf_id, ca.next_mp_id, ca.outlier_mps) == (cb.next_kf_id, cb.next_mp_id, cb.outlier_mps)
    print(f"composition: {turns} device turns per stream over {STEPS} steps, {dev.trk.keyframe_launches()} launches per turn")


def test_turn_insert_optimise_update_step(api, pkg, synth):
    import torch
    chain = pkg.chain
    S, KFC, MPC, OBC, WINDOW = 3, 8, 512, 2048, 7
    rig = Rig(api, S, good=20, bad=-1)
    be = api.Backend(S, KFC, MPC, OBC)
    z = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device="cuda")
    T = {"kf_id": z((S, KFC), "int64"), "kf_pose": z((S, KFC, 7), "float64"), "n_kf": z((S,), "int32"), "mp_id": z((S, MPC), "int64"),
         "mp_pos": z((S, MPC, 3), "float64"), "mp_outlier": z((S, MPC), "uint8"), "n_mp": z((S,), "int32"), "obs_mp": z((S, OBC), "int32"),
         "obs_kf": z((S, OBC), "int32"), "obs_flags": z((S, OBC), "uint8"), "obs_uv": z((S, OBC, 2), "float32"), "obs_tag": z((S, OBC), "int32"),
         "n_obs": z((S,), "int32")}
    order = ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")
    I = {"feat_row": z((S, rig.cap), "int32"), "mp_new_row": z((S, MPC), "int32"), "removed_kf_id": z((S,), "int64"), "removed_kf_row": z((S,), "int32"),
         "dis": z((S, KFC), "float64"), "status": z((S,), "int32")}
    O = {"obs_report": z((S, OBC), "uint8"), "mp_report": z((S, MPC), "uint8"), "new_outlier": z((S, MPC), "int32"), "n_new": z((S,), "int32"),
         "obs_chi2": z((S, OBC), "float64"), "rounds": z((S,), "int32"), "n_out": z((S,), "int32"), "status": z((S,), "int32")}
    # the tables hold each stream's reference key-frame (id 7, the state's ref pose) and its landmarks, as after StereoInit; stream 2 takes no turn
    cases = [KC.rich_case(chain, synth), KC.total_case(chain, synth, 65), KC.make(chain, synth, "idle", n=20, n_new=4, seed=260)]
    for s, c in enumerate(cases):
        rig.load(s, c, why=KR.WHY_KEYFRAME if s < 2 else KR.WHY_LOST)
        lid = c["ids"]["landmark_id"]
        T["kf_id"][s, 0] = 7; T["kf_pose"][s, 0] = torch.from_numpy(np.asarray(c["st"]["ref_pose"], float)); T["n_kf"][s] = 1
        T["mp_id"][s, :len(lid)] = torch.from_numpy(lid); T["mp_pos"][s, :len(lid)] = torch.from_numpy(np.asarray(c["st"]["lm_pos"], float)); T["n_mp"][s] = len(lid)
        T["mp_outlier"][s, :len(lid)] = torch.from_numpy(np.asarray(c["st"]["lm_outlier"], np.uint8))
        Tref = chain.T_of(c["st"]["ref_pose"])              # key-frame 7 observes every landmark where it projects (one ACTIVE row each, in id order)
        pc = np.array([chain.mv(Tref[:3, :3], p) + Tref[:3, 3] for p in c["st"]["lm_pos"]])
        uv = np.stack([rig.K[0] * pc[:, 0] / pc[:, 2] + rig.K[2], rig.K[1] * pc[:, 1] / pc[:, 2] + rig.K[3]], 1).astype(np.float32)
        T["obs_mp"][s, :len(lid)] = torch.arange(len(lid), dtype=torch.int32); T["obs_flags"][s, :len(lid)] = 1; T["obs_uv"][s, :len(lid)] = torch.from_numpy(uv)
        T["obs_tag"][s, :len(lid)] = torch.arange(len(lid), dtype=torch.int32); T["n_obs"][s] = len(lid)
    before = {k: v.cpu().numpy().copy() for k, v in T.items()}
    out = rig.turn()
    assert out["report"][:, 0].tolist() == [0, 0, api.Tracker.NO_TURN] and out["new_kf_id"].tolist() == [12, 12, -1]
    be.insert_keyframe_batch(*[T[k].data_ptr() for k in order], *[rig.out[k].data_ptr() for k in ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos",
                             "feat_uv", "feat_tag", "feat_flags", "n_feat")], rig.cap, 0, 0, 0, 0, 0, 0, 1, rig.out["outlier_mp_id"].data_ptr(),
                             rig.out["n_outlier_mp"].data_ptr(), 2 * rig.cap, S, WINDOW, 0.2, *[I[k].data_ptr() for k in ("feat_row", "mp_new_row",
                             "removed_kf_id", "removed_kf_row", "dis", "status")])
    torch.cuda.synchronize()
    # a no-turn item (id -1, no features) on a table that holds a key-frame: refused, every byte kept (the header says so)
    assert I["status"].cpu().numpy().tolist() == [0, 0, api.ERR_INVALID]
    after = {k: v.cpu().numpy() for k, v in T.items()}
    assert all(_same(after[k][2], before[k][2]) for k in T) and after["n_kf"].tolist() == [2, 2, 1]
    assert after["n_mp"][0] == len(cases[0]["ids"]["landmark_id"]) + out["report"][0, 4]          # every new map point entered the table
    be.optimize_batch(*[T[k].data_ptr() for k in order], S, rig.K, *[O[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2",
                      "rounds", "n_out", "status")])
    rig.trk.update_from_map(T["kf_id"].data_ptr(), T["kf_pose"].data_ptr(), T["n_kf"].data_ptr(), KFC, T["mp_id"].data_ptr(), T["mp_pos"].data_ptr(),
                            T["mp_outlier"].data_ptr(), T["n_mp"].data_ptr(), MPC)
    d_res = torch.zeros(S * 80, dtype=torch.uint8, device="cuda")
    d_img = torch.from_numpy(np.stack([c["left"] for c in cases])).cuda()
    rig.trk.step_batch(d_img.data_ptr(), rig.cols, rig.rows * rig.cols, d_res.data_ptr())
    torch.cuda.synchronize()
    assert O["status"].cpu().numpy()[:2].tolist() == [0, 0]
    tab = {k: v.cpu().numpy() for k, v in T.items()}
    res = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    for s in range(2):
        st, ids = rig.trk.get_frame(s), rig.trk.get_ids(s)
        rows = {int(i): r for r, i in enumerate(tab["mp_id"][s, :tab["n_mp"][s]])}
        held = [l for l, i in enumerate(ids["landmark_id"]) if int(i) in rows]
        assert len(held) >= out["report"][s, 6] // 2 and all(_same(st["lm_pos"][l], tab["mp_pos"][s, rows[int(ids["landmark_id"][l])]]) for l in held)
        assert all(st["lm_outlier"][l] == tab["mp_outlier"][s, rows[int(ids["landmark_id"][l])]] for l in held)
        assert _same(st["ref_pose"], tab["kf_pose"][s, list(tab["kf_id"][s, :tab["n_kf"][s]]).index(12)])
        assert res["status"][s] in (chain.TRACKING_GOOD, chain.TRACKING_BAD) and res["frame_id"][s] == 10 and res["n_features"][s] >= 30
    assert rig.trk.get_frame(2)["frozen"] == 1
    # ... and on an EMPTY key-frame table there is no last id to refuse it by: the row (-1) is appended, as the header warns
    E = {k: torch.zeros_like(v) for k, v in T.items()}
    be.insert_keyframe_batch(*[E[k].data_ptr() for k in order], *[rig.out[k].data_ptr() for k in ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos",
                             "feat_uv", "feat_tag", "feat_flags", "n_feat")], rig.cap, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, S, WINDOW, 0.2,
                             *[I[k].data_ptr() for k in ("feat_row", "mp_new_row", "removed_kf_id", "removed_kf_row", "dis", "status")])
    torch.cuda.synchronize()
    assert I["status"].cpu().numpy()[2] == 0 and E["n_kf"].cpu().numpy()[2] == 1 and E["kf_id"].cpu().numpy()[2, 0] == -1
