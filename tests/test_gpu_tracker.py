"""The multi-stream tracker (csrc/tracker.hip, api.Tracker, chain.StreamBank) on the GPU, checked in LOCK-STEP against tests/tracker_ref.py
(the step restated with the oracle's operators, itself checked against Chain(OracleBackend) in tests/test_tracker_ref.py): before every step each
stream's state is downloaded, the expected step is computed from THAT state, the device's result is compared and the run continues from the
device's state.  Two free-running chains are not bit-comparable (tests/oracle_backend.py:73-78).

Figures measured on an MI355X are printed by each test (pytest -s); see DESIGN.md §3.20."""
import numpy as np
import pytest

import tracker_ref as TR
from chain_compare import compare_runs
from oracle_backend import CheckedBackend, OracleBackend

pytestmark = pytest.mark.gpu

CFG = {"numFeatures.trackingGood": 390}
OFFSETS = [0, 3, 7, 11, 16, 20, 25, 29]          # where in the rendered sequence each stream starts
KF_EVERY = [0, 0, 0, 0, 0, 0, 6, 6]
LATE = {7: 5}                                     # stream 7 is initialised 5 steps after the others: never set = frozen until then
STEPS = 64
_cache = {}


def _frames(synth):
    if "frames" not in _cache:
        scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
        _cache["frames"] = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(max(OFFSETS) + STEPS + 8)]
    return _cache["frames"]


class _DeviceResult:
    """the device's pose-only result behind the back-end interface, so that CheckedBackend.pose_only (the bar and its budget) judges it"""
    def pose_only(self, pose, p3, obs, Kt, pre=0):
        return self.result


def _bank(pkg, api, synth, offsets, kf_every, late=None):
    chain = pkg.chain
    frames = _frames(synth)
    lcd = api.DeepLCD(synth.calc_weights_handcrafted())
    late = late or {}
    mk = lambda o, d: (lambda t: frames[o + t - d] if t >= d else frames[o])
    chains = [chain.Chain(chain.HipBackend(api, cfg=CFG, lcd=lcd), api, synth.SEQ_K, mk(o, late.get(s, 0)), cfg=CFG, kf_every=kf_every[s], log=False)
              for s, o in enumerate(offsets)]
    return chain.StreamBank(chains, api, cap=1024, landmark_cap=2048)


def _run(pkg, api, synth, oracle, offsets, kf_every, steps, late=None, check=True):
    """lock-step run; returns (trace[k][s] = (record, p1 bytes, tracked bytes), counters, checker)"""
    chain = pkg.chain
    late = late or {}
    bank = _bank(pkg, api, synth, offsets, kf_every, late)
    trk, S = bank.trk, len(offsets)
    K, good, bad = bank.chains[0].Kt, bank.chains[0].n_good, bank.chains[0].n_bad
    dev = _DeviceResult()
    chk = CheckedBackend(dev, OracleBackend(oracle, None, CFG, chain))
    cnt = {"bad_keyframes": 0, "kf_every_keyframes": 0, "fresh_outliers": 0, "frozen_steps": 0, "lost": 0, "stream_steps": 0}
    trace = []
    for k in range(steps + 1):
        bank.upload(k)
        on = [s for s in range(S) if bank.on_device[s]]
        pre = {s: trk.get_frame(s, image=True) for s in on} if check else {}
        idle = {s: (trk.get_frame(s), bank.results()[s].tobytes()) for s in range(S) if s not in on} if check and on else {}
        row = {}
        if on:
            bank.step()
            res = bank.results()
        for s in idle:                                   # frozen (never set) streams: state and record untouched by the step
            assert trk.get_frame(s)["frozen"] == 1 and bank.results()[s].tobytes() == idle[s][1]
            assert all(np.array_equal(trk.get_frame(s)[key], idle[s][0][key]) for key in ("xy", "lm", "last_rel", "rel_motion"))
            cnt["frozen_steps"] += 1
        for s in on:
            rec = res[s]
            p0, p1, nxt, lk_st = trk.debug_last_step(s)
            row[s] = (rec.copy(), p1.tobytes(), nxt[lk_st].tobytes())
            cnt["stream_steps"] += 1
            if check:
                post = trk.get_frame(s)
                _, _, e = TR.step(chain, oracle, K, pre[s], pre[s]["image"], bank.images[s][0], good, bad)
                tag = f"step {k} stream {s}"
                assert p0.tobytes() == e["p0"].tobytes() and p1.tobytes() == e["p1"].tobytes(), tag + ": LK start points are not the host's bits"
                assert np.array_equal(lk_st, e["lk_status"]) and nxt[lk_st].tobytes() == e["nxt"][e["lk_status"]].tobytes(), tag + ": LK status / tracks"
                assert post["xy"].tobytes() == e["xy"].tobytes(), tag + ": current feature table"
                d_outl = np.array([post["lm"][j] < 0 for j in range(len(e["po"])) if e["po"][j] >= 0], bool)
                dev.result = (rec["pose7"].copy(), d_outl, int(rec["n_inliers"]))
                chk.pose_only(e["pose0"], e["p3"], e["obs"], K)                  # rtol = atol = 1e-6, flags equal, else the budgeted one-ulp rule
                # rules 5 + 6 recomputed from what the device accepted: equal bits
                new, r2 = TR.finish(chain, pre[s], e["xy"], e["lm"], e["po"], rec["pose7"], d_outl, int(rec["n_inliers"]), good, bad)
                assert np.array_equal(post["lm"], new["lm"]) and np.array_equal(post["lm_outlier"], new["lm_outlier"]), tag + ": landmark flags"
                assert np.array_equal(post["outlier_list"], new["outlier_list"]), tag + ": outlier-landmark list"
                assert (int(rec["status"]), int(rec["needs_host"]), int(rec["frame_id"]), int(rec["n_features"])) == \
                       (r2["status"], r2["needs_host"], r2["frame_id"], r2["n_features"]), tag + ": record"
                assert post["frozen"] == r2["needs_host"] and post["next_frame_id"] == pre[s]["next_frame_id"] + 1 and post["status"] == r2["status"]
                Tref = chain.T_of(pre[s]["ref_pose"])
                assert chain.p7_of(chain.mm(post["last_rel"], Tref)).tobytes() == rec["pose7"].tobytes(), tag + ": record pose vs rel"
                assert chain.mm(post["last_rel"], chain.T_inv(pre[s]["last_rel"])).tobytes() == post["rel_motion"].tobytes(), tag + ": relative motion"
                # (the raw optimiser pose is not exported: rel = T(pose) T(ref)^-1 is checked through the record's pose, to rounding)
                assert np.abs(chain.mm(chain.T_of(rec["pose7"]), chain.T_inv(Tref)) - post["last_rel"]).max() < 1e-12
                cnt["fresh_outliers"] += len(new["outlier_list"]) - len(pre[s]["outlier_list"])
            c = bank.chains[s]
            if rec["needs_host"]:
                if rec["status"] == chain.LOST:
                    cnt["lost"] += 1
                elif c.kf_every > 0:
                    cnt["kf_every_keyframes"] += 1
                else:
                    assert rec["status"] == chain.TRACKING_BAD
                    cnt["bad_keyframes"] += 1
                bank.host_turn(s, rec, k)
            else:
                c.status = int(rec["status"]); c.next_frame_id = int(rec["frame_id"]) + 1
                c.poses.append(rec["pose7"].copy())
        for s in range(S):
            c = bank.chains[s]
            if s not in on and c.status == chain.INITING and k >= late.get(s, 0):
                c.grab(k)
                assert c.status == chain.TRACKING_GOOD
                bank.hand_off(s)
        trace.append(row)
    return trace, cnt, chk, bank


def test_lock_step_parity_8_streams(api, pkg, synth, oracle):
    trace, cnt, chk, bank = _run(pkg, api, synth, oracle, OFFSETS, KF_EVERY, STEPS, LATE)
    _cache["trace8"] = trace
    print(f"tracker lock-step: {cnt}, {bank.trk.launches_per_step()} launches per step, pose-only calls {chk.calls.get('pose_only')}, "
          f"soft-bar uses {getattr(chk, 'soft', {})}, largest deviations {({k: float(f'{v:.2e}') for k, v in chk.dev.items()})}")
    assert cnt["stream_steps"] >= 8 * 60 - LATE[7] - 8 and cnt["lost"] == 0
    assert cnt["bad_keyframes"] >= 6 and cnt["kf_every_keyframes"] >= 10, cnt          # TRACKING_BAD -> key-frame by the reference's rule; kf_every 6
    assert cnt["fresh_outliers"] >= 1, cnt                                            # the `<= 2` rule marked landmarks
    assert cnt["frozen_steps"] >= LATE[7] - 1, cnt                                    # steps that passed a frozen stream
    kfs = [c.kf_frames for c in bank.chains]
    assert len({tuple(k) for k in kfs[:6]}) > 1                                      # the key-frames fall on different steps


def test_stream_results_do_not_depend_on_the_bank(api, pkg, synth, oracle):
    """stream 2 of the bank of 8 against the same stream as a bank of 1: LK start points and tracks bitwise, pose at the batch-against-single bar
    of tests/test_gpu_pose_only.py (rtol 1e-8, atol 1e-9), counts and decisions equal"""
    if "trace8" not in _cache:
        _cache["trace8"] = _run(pkg, api, synth, oracle, OFFSETS, KF_EVERY, STEPS, LATE, check=False)[0]
    one = _run(pkg, api, synth, oracle, [OFFSETS[2]], [KF_EVERY[2]], STEPS, check=False)[0]
    n, worst = 0, 0.0
    for k, (r8, r1) in enumerate(zip(_cache["trace8"], one)):
        if 2 not in r8:
            assert 0 not in r1
            continue
        (a, ap1, anx), (b, bp1, bnx) = r8[2], r1[0]
        assert ap1 == bp1 and anx == bnx, f"step {k}: LK"
        assert np.allclose(a["pose7"], b["pose7"], rtol=1e-8, atol=1e-9), (k, np.abs(a["pose7"] - b["pose7"]).max())
        assert all(a[f] == b[f] for f in ("n_inliers", "n_features", "status", "frame_id", "needs_host")), k
        worst = max(worst, float(np.abs(a["pose7"] - b["pose7"]).max())); n += 1
    print(f"S-independence: {n} steps, largest pose deviation {worst:.2e}")
    assert n >= 60


def _two_stream_setup(api, pkg, synth, kf_every):
    import torch
    bank = _bank(pkg, api, synth, [0, 11], kf_every)
    for s, c in enumerate(bank.chains):
        c.grab(0)
    states = [TR.state_of_chain(pkg.chain, c, c.kf_every)[0] for c in bank.chains]
    imgs = [c.cur.L for c in bank.chains]
    return bank, states, imgs, torch


def _dump(trk, bank, S):
    out = [bank.results().tobytes()]
    for s in range(S):
        st = trk.get_frame(s, image=True)
        out += [np.asarray(st[k]).tobytes() for k in sorted(st)]
    return out


def test_frozen_stream_is_untouched(api, pkg, synth):
    bank, states, imgs, torch = _two_stream_setup(api, pkg, synth, [1, 1000])         # stream 0: key-frame at every frame -> frozen by the first step; stream 1: none
    for s in range(2):
        bank.trk.set_frame(s, states[s], image=imgs[s])
    bank.upload(1); bank.step()
    r = bank.results()
    assert r[0]["needs_host"] == 1 and r[1]["needs_host"] == 0 and bank.trk.get_frame(0)["frozen"] == 1
    before = _dump(bank.trk, bank, 1)[1:] + [r[0].tobytes()]
    for k in (2, 3, 4):
        bank.upload(k); bank.step()
    r2 = bank.results()
    assert _dump(bank.trk, bank, 1)[1:] + [r2[0].tobytes()] == before, "a frozen stream's state, image or record changed"
    assert r2[1]["frame_id"] == r[1]["frame_id"] + 3 and bank.trk.debug_last_step(0)[0].shape[0] == 0


def test_recorded_step_equals_eager_step(api, pkg, synth):
    bank, states, imgs, torch = _two_stream_setup(api, pkg, synth, [0, 0])
    s_main, s_side = torch.cuda.Stream(), torch.cuda.Stream()
    bank.trk.set_stream(s_main.cuda_stream)
    bank.upload(1); torch.cuda.synchronize()

    def reset():
        for s in range(2):
            bank.trk.set_frame(s, states[s], image=imgs[s])
    reset(); bank.step(); torch.cuda.synchronize()
    eager = _dump(bank.trk, bank, 2)
    reset()
    bank.d_res.zero_(); torch.cuda.synchronize()
    g = api.StepGraph.record(s_main.cuda_stream, [s_side.cuda_stream], bank.step)
    assert g.node_count() >= bank.trk.launches_per_step()
    assert bank.results().tobytes() == bytes(len(eager[0])), "recording a step must not run it"
    g.launch(s_main.cuda_stream); torch.cuda.synchronize()
    assert _dump(bank.trk, bank, 2) == eager
    assert bank.results()[0]["n_features"] > 100


def test_capacity_and_empty_streams(api, pkg, synth):
    bank, states, imgs, torch = _two_stream_setup(api, pkg, synth, [0, 0])
    chain = pkg.chain
    small = api.Tracker(3, bank.rows, bank.cols, 64, 2048, bank.chains[0].Kt, 390, 10)          # cap 64 < the ~300 features of stream 0
    with pytest.raises(api.MyslamError) as e:
        small.set_frame(0, states[0], image=imgs[0])
    assert e.value.code == api.ERR_CAPACITY
    few = dict(states[1]); few["xy"], few["lm"] = states[1]["xy"][:60], states[1]["lm"][:60]
    small.set_frame(1, few, image=imgs[1])
    empty = dict(states[1]); empty["xy"], empty["lm"] = np.zeros((0, 2), np.float32), np.zeros(0, np.int32)
    small.set_frame(2, empty, image=imgs[1])
    d_img = torch.from_numpy(np.stack([bank.chains[0].frame_images(1)[0], bank.chains[1].frame_images(1)[0], bank.chains[1].frame_images(1)[0]])).cuda()
    d_res = torch.zeros(3 * 80, dtype=torch.uint8, device="cuda")
    small.step_batch(d_img.data_ptr(), bank.cols, bank.rows * bank.cols, d_res.data_ptr())
    r = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert r[0]["status"] == api.ERR_CAPACITY and r[0]["needs_host"] == 1 and r[0]["n_features"] == 0 and small.get_frame(0)["frozen"] == 1
    assert r[1]["status"] in (chain.TRACKING_GOOD, chain.TRACKING_BAD, chain.LOST) and 0 < r[1]["n_features"] <= 60 and r[1]["n_inliers"] <= 60
    assert r[2]["status"] == chain.LOST and r[2]["n_inliers"] == 0 and r[2]["n_features"] == 0 and r[2]["needs_host"] == 1
    # the stream beside the overflowing one is what it is alone
    alone = api.Tracker(1, bank.rows, bank.cols, 64, 2048, bank.chains[0].Kt, 390, 10)
    alone.set_frame(0, few, image=imgs[1])
    d_res1 = torch.zeros(80, dtype=torch.uint8, device="cuda")
    alone.step_batch(d_img[1:].data_ptr(), bank.cols, bank.rows * bank.cols, d_res1.data_ptr())
    assert d_res1.cpu().numpy().tobytes() == r[1].tobytes()


def test_stream_bank_composition_4_streams(api, pkg, synth):
    """chain.StreamBank over 4 streams x 120 frames against 4 separate Chain(HipBackend) runs at the free-run bars of tests/test_gpu_sequence.py"""
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(120 + 24)]
    cfg = dict(CFG, **{"LCD.nDatabaseMinSize": 25})          # one handle = one pair of thresholds for all its streams
    w = synth.calc_weights_handcrafted()
    offs, kfe = [0, 6, 13, 24], [6, 6, 0, 0]
    mk = lambda o: [frames[o + t] for t in range(120)]
    new = lambda s: chain.Chain(chain.HipBackend(api, w, cfg), api, synth.SEQ_K, mk(offs[s]), cfg=cfg, kf_every=kfe[s], correct_threshold=0.0)
    bank = chain.StreamBank([new(s) for s in range(4)], api, cap=1024, landmark_cap=2048).run(120)
    for s in range(4):
        a, b = bank.chains[s], new(s).run()
        rep = compare_runs(a, b)
        print(f"stream bank, stream {s}: {len(a.kf_frames)} key-frames, {rep}")
        assert len(a.poses) == len(b.poses) == 120 and rep["diverged_at"] is None
        assert rep["same_key_frames"] and rep["same_loops"] and rep["tracks"] > 10000 and rep["tracks_within_0.03px"] >= 0.99 * rep["tracks"]
        assert rep["frame_pose_max_dev"] < 1e-4 and rep["pose_max_dev"] < 1e-4
    assert bank.steps == 119
