"""tests/tracker_ref.py (the multi-stream tracker's step restated on plain arrays) is itself checked: driven frame by frame beside
Chain(OracleBackend).track() on the 44-frame run of tests/test_chain_host.py (720 x 240, numFeatures.trackingGood 390: the reference's own rule
inserts 8 key-frames) it reproduces the chain's LK start points, feature lists, poses, statuses, outlier-landmark list and key-frame decisions
bit for bit — the same operators in the same order, so equality, no tolerance.  CPU only."""
import numpy as np

import tracker_ref as TR
from oracle_backend import OracleBackend

CFG = {"numFeatures.trackingGood": 390}
N = 44


def _feat_list(c):
    return [(np.float32(f.x).tobytes(), np.float32(f.y).tobytes(), f.mp.id if f.live() is not None else None) for f in c.cur.feats]


def test_restatement_reproduces_the_chain_bit_for_bit(pkg, synth, oracle):
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(N)]
    c = chain.Chain(OracleBackend(oracle, synth.calc_weights_handcrafted(), CFG, chain), pkg.api, synth.SEQ_K, frames, cfg=CFG)
    K = c.Kt
    assert c.grab(0) and c.status == chain.TRACKING_GOOD
    st, ids = TR.state_of_chain(chain, c)
    n_kf = n_fresh = n_plain = 0
    for t in range(1, N):
        prev = c.last.L                                   # the key-frame's image after DeepLCD blurred it in place, where it did
        n_log, n_out = len(c.log), len(c.outlier_mps)
        new, rec, dbg = TR.step(chain, oracle, K, st, prev, frames[t][0], c.n_good, c.n_bad)
        assert c.grab(t)
        log = dict((tag, x) for tag, x in c.log[n_log:n_log + 2])
        nxt, lk_st, p1 = log["lk_track"]
        assert p1.tobytes() == dbg["p1"].tobytes(), f"frame {t}: LK start points"
        assert np.array_equal(lk_st.astype(bool), dbg["lk_status"]) and nxt.tobytes() == dbg["nxt"].tobytes()
        pose, outl, ninl = log["pose_only"]
        assert pose.tobytes() == dbg["pose"].tobytes() and np.array_equal(outl.astype(bool), dbg["outlier"]) and int(ninl[0]) == rec["n_inliers"]
        assert c.status == rec["status"] and c.cur.id == rec["frame_id"]
        assert np.asarray(c.rel_motion).tobytes() == new["rel_motion"].tobytes(), f"frame {t}: relative motion"
        is_kf = c.kf_frames[-1] == c.cur.id
        assert is_kf == bool(rec["needs_host"]) == (rec["status"] == chain.TRACKING_BAD), f"frame {t}: key-frame decision"
        if is_kf:                                         # the host's turn: new features, new landmarks, local BA — the state is handed over again
            n_kf += 1
            st, ids = TR.state_of_chain(chain, c)
            continue
        n_plain += 1
        assert np.asarray(c.poses[-1]).tobytes() == rec["pose7"].tobytes() and np.asarray(c.cur.rel).tobytes() == new["last_rel"].tobytes()
        assert _feat_list(c) == [(x.tobytes(), y.tobytes(), ids[l] if l >= 0 else None) for (x, y), l in zip(new["xy"], new["lm"])], f"frame {t}: feature list"
        added = [ids[l] for l in new["outlier_list"][len(st["outlier_list"]):]]
        assert c.outlier_mps[n_out:] == added, f"frame {t}: outlier map points"
        assert [1 if c.all_mps[m].outlier else 0 for m in ids] == new["lm_outlier"].tolist()
        n_fresh += len(added)
        st = new
    assert n_kf == len(c.kf_frames) - 1 >= 7 and n_plain > 20 and n_fresh > 0, (n_kf, n_plain, n_fresh)


def test_kf_every_rule_and_lost(pkg):
    chain = pkg.chain
    st = {"xy": np.zeros((0, 2), np.float32), "lm": np.zeros(0, np.int32), "lm_pos": np.zeros((0, 3)), "lm_outlier": np.zeros(0, np.uint8),
          "ref_pose": chain.IDENT.copy(), "ref_frame_id": 0, "last_rel": np.eye(4), "rel_motion": np.eye(4), "next_frame_id": 6, "status": 1,
          "kf_every": 6, "frozen": 0, "outlier_list": np.zeros(0, np.int32)}
    e = np.zeros(0, np.int32)
    for ninl, fid, kfe, want in [(400, 6, 6, (1, 1)), (400, 7, 6, (1, 0)), (100, 7, 6, (2, 0)), (100, 7, 0, (2, 1)), (5, 12, 6, (3, 1)), (5, 7, 0, (3, 1))]:
        new, rec = TR.finish(chain, dict(st, next_frame_id=fid, kf_every=kfe), st["xy"], e, e, chain.IDENT, np.zeros(0, bool), ninl, 390, 10)
        assert (rec["status"], rec["needs_host"]) == want and new["frozen"] == want[1] and new["next_frame_id"] == fid + 1
