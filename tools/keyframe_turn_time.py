"""Times the key-frame turn of the multi-stream tracker on the GPU box for 16 and 64 eligible streams at 1241 x 376 with about 150 kept features
(each on a landmark) and the key-points the extractor finds under the turn's mask (ORBextractor(150): about 150):

  device   Tracker.keyframe_masks -> ORBextractor.detect_batch -> Tracker.keyframe_batch, three asynchronous calls on one stream, one synchronise;
  host     the same turns the way chain.StreamBank.host_turn takes them, in the same library: per stream get_frame, the mask in numpy, the three
           synchronous single-image calls (ORBextractor.Detect, LKTracker.track, triangulate_stereo), the tables rebuilt in Python (first-reference
           slots), set_frame + set_ids.

Before every timed call the streams are put back into the same frozen state (set_frame, set_ids and the freeze: not timed).  Host clock around spans
that end in a synchronise; both forms warmed up, then timed REPS times in alternation; medians with min - max go to
profiles/keyframe_turn_time.json (--out names another file).  There is no pass / fail ratio: the tool reports what it reads."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_turn_time.json"))
ap.add_argument("--streams", type=int, nargs="+", default=[16, 64])
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api, chain, synth = pkg.api, pkg.chain, pkg.synth
ROWS, COLS, NKEPT, NNEW, CAP, LM_CAP, D = 376, 1241, 150, 150, 512, 1024, 4
K = (718.856, 718.856, 607.1928, 185.2157); BASE = 0.537
DEPTH = K[0] * BASE / D


def stream_case(seed):
    """a stream frozen at a key-frame: NKEPT features on landmarks DEPTH in front of the identity pose, the right image = the left moved by D pixels"""
    rng = np.random.default_rng([seed, 0x7F])
    big = synth.random_image(seed, ROWS + 16, COLS + 16, "texture")
    left, right = np.ascontiguousarray(big[8:8 + ROWS, 8:8 + COLS]), np.ascontiguousarray(big[8:8 + ROWS, 8 + D:8 + D + COLS])
    xy = np.stack([rng.uniform(30, COLS - 31, NKEPT), rng.uniform(30, ROWS - 31, NKEPT)], 1).astype(np.float32)
    pos = np.stack([(xy[:, 0] - K[2]) / K[0] * DEPTH, (xy[:, 1] - K[3]) / K[1] * DEPTH, np.full(NKEPT, DEPTH)], 1).astype(np.float64)
    st = {"xy": xy, "lm": np.arange(NKEPT, dtype=np.int32), "lm_pos": pos, "lm_outlier": np.zeros(NKEPT, np.uint8), "ref_pose": chain.IDENT.copy(),
          "ref_frame_id": 4, "last_rel": np.eye(4), "rel_motion": np.eye(4), "next_frame_id": 10, "status": 1, "kf_every": 0}
    return st, 100 + np.arange(NKEPT, dtype=np.int64), left, right


def host_turn(trk, orb, lk, s, left, right):
    """one stream's turn through the host: the steps of Chain.detect_features / find_features_in_right / triangulate_new_points / insert_keyframe and
    StreamBank.hand_off on arrays"""
    st, ids = trk.get_frame(s), trk.get_ids(s)
    mask = np.full((ROWS, COLS), 255, np.uint8)
    for x, y in st["xy"]:
        x0, x1 = int(np.rint(np.float32(x - np.float32(20)))), int(np.rint(np.float32(x + np.float32(20))))
        y0, y1 = int(np.rint(np.float32(y - np.float32(20)))), int(np.rint(np.float32(y + np.float32(20))))
        mask[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = 0
    new = orb.Detect(left, mask)
    p0 = np.concatenate([st["xy"], np.stack([new["x"], new["y"]], 1).astype(np.float32)])
    lm = np.concatenate([st["lm"], np.full(len(new), -1, np.int32)])
    Tcw = chain.mm(st["last_rel"], chain.T_of(st["ref_pose"]))
    p1 = p0.copy()
    for i, l in enumerate(lm):
        if l >= 0 and not st["lm_outlier"][l]:
            pc = chain.mv(Tcw[:3, :3], st["lm_pos"][l]) + Tcw[:3, 3] + np.array([-BASE, 0.0, 0.0])
            p1[i] = (K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3])
    nxt, ok, _ = lk.track(left, right, p0, p1)
    cand = [i for i in range(len(lm)) if lm[i] < 0 and ok[i]]
    xyz, tok = api.triangulate_stereo(p0[cand, 0], p0[cand, 1], nxt[cand, 0], nxt[cand, 1], *K, BASE) if cand else (np.zeros((0, 3)), np.zeros(0, bool))
    Twc = chain.T_inv(Tcw)
    fid = [int(ids["landmark_id"][l]) if l >= 0 else -1 for l in lm]
    fpos = [st["lm_pos"][l] if l >= 0 else None for l in lm]
    fout = [st["lm_outlier"][l] if l >= 0 else 0 for l in lm]
    nmp = ids["next_mp_id"]
    for j, i in enumerate(cand):
        if tok[j]:
            fid[i], fpos[i] = nmp, chain.mv(Twc[:3, :3], xyz[j]) + Twc[:3, 3]; nmp += 1
    slot, nid, npos, nout, nlm = {}, [], [], [], np.full(len(lm), -1, np.int32)
    for i, m in enumerate(fid):
        if m >= 0:
            if m not in slot:
                slot[m] = len(nid); nid.append(m); npos.append(fpos[i]); nout.append(fout[i])
            nlm[i] = slot[m]
    new_st = dict(st, xy=p0, lm=nlm, lm_pos=np.array(npos, float).reshape(-1, 3), lm_outlier=np.array(nout, np.uint8), ref_pose=chain.p7_of(Tcw),
                  ref_frame_id=st["next_frame_id"] - 1, last_rel=np.eye(4))
    trk.set_frame(s, new_st, image=left)
    trk.set_ids(s, nid, ids["next_kf_id"], ids["next_kf_id"] + 1, nmp)
    return len(new), int(np.count_nonzero(ok)), nmp - ids["next_mp_id"]


def measure(S):
    made = [stream_case(100 + s) for s in range(S)]
    stream = torch.cuda.Stream()
    trk = api.Tracker(S, ROWS, COLS, CAP, LM_CAP, K, stream=stream.cuda_stream)
    orb, lk = api.ORBextractor(NNEW, stream=stream.cuda_stream), api.LKTracker()
    kp_cap = int(orb.max_keypoints(ROWS, COLS))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    out = {"new_kf_id": z(S, torch.int64), "new_kf_pose": z((S, 7), torch.float64), "feat_mp_id": z((S, CAP), torch.int64), "feat_mp_pos": z((S, CAP, 3), torch.float64),
           "feat_uv": z((S, CAP, 2), torch.float32), "feat_tag": z((S, CAP), torch.int32), "feat_flags": z((S, CAP), torch.uint8), "n_feat": z(S, torch.int32),
           "outlier_mp_id": z((S, 2 * CAP), torch.int64), "n_outlier_mp": z(S, torch.int32), "right_xy": z((S, CAP, 2), torch.float32),
           "right_ok": z((S, CAP), torch.uint8), "report": z((S, 8), torch.int32)}
    d_left = torch.from_numpy(np.stack([m[2] for m in made])).cuda(); d_right = torch.from_numpy(np.stack([m[3] for m in made])).cuda()
    d_mask = z((S, ROWS, COLS), torch.uint8); d_kps = z((S, kp_cap, 28), torch.uint8); d_n = z(S, torch.int32); d_st = z(S, torch.int32)
    torch.cuda.synchronize()
    img = ROWS * COLS

    def reset():
        for s, (st, lid, left, _) in enumerate(made):
            trk.set_frame(s, st, image=left); trk.set_ids(s, lid, 7, 12, 1000); trk.debug_freeze(s, 1)

    def device():
        trk.keyframe_masks(d_mask.data_ptr(), COLS, img)
        orb.detect_batch(d_left.data_ptr(), S, ROWS, COLS, COLS, img, d_kps.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), kp_cap, d_masks=d_mask.data_ptr())
        trk.keyframe_batch(d_right.data_ptr(), COLS, img, d_kps.data_ptr(), d_n.data_ptr(), kp_cap, BASE, {k: v.data_ptr() for k, v in out.items()})
        stream.synchronize()

    def host():
        return [host_turn(trk, orb, lk, s, made[s][2], made[s][3]) for s in range(S)]

    def timed(fn):
        reset()
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    for fn in (device, host):
        timed(fn)
    times = {"device": [], "host": []}
    for _ in range(args.reps):
        times["device"].append(timed(device)[0])
        ms, counts = timed(host)
        times["host"].append(ms)
    reset(); device()
    rep = out["report"].cpu().numpy()
    assert (rep[:, 0] == 0).all(), rep[:, 0]
    hc = np.array(counts)
    res = {"streams": S, "device_counts": {"detected": [int(rep[:, 2].min()), int(rep[:, 2].max())], "right_matches": [int(rep[:, 3].min()), int(rep[:, 3].max())],
                                           "new_map_points": [int(rep[:, 4].min()), int(rep[:, 4].max())], "features": [int(rep[:, 5].min()), int(rep[:, 5].max())]},
           "host_counts": {"detected": [int(hc[:, 0].min()), int(hc[:, 0].max())], "right_matches": [int(hc[:, 1].min()), int(hc[:, 1].max())],
                           "new_map_points": [int(hc[:, 2].min()), int(hc[:, 2].max())]},
           "launches": {"masks": 1, "turn": trk.keyframe_launches()}, "ms": {}}
    for k, v in times.items():
        res["ms"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
        print(f"{S:3d} streams  {k:7s} median {np.median(v):10.3f} ms   (min {min(v):.3f}, max {max(v):.3f}, {args.reps} calls)", flush=True)
    res["host_over_device"] = res["ms"]["host"]["median"] / res["ms"]["device"]["median"]
    res["clock_mhz"] = float(api.shader_clock_mhz(stream.cuda_stream))
    return res


result = {"workload": f"{ROWS} x {COLS}, {NKEPT} kept features, ORBextractor({NNEW}) under the mask, cap {CAP}, landmark cap {LM_CAP}, disparity {D} px",
          "calls_per_form": args.reps, "runs": [measure(S) for S in args.streams], "build": api.build_id()}
for r in result["runs"]:
    print(f"{r['streams']} streams: host {r['ms']['host']['median']:.1f} ms, device {r['ms']['device']['median']:.2f} ms: {r['host_over_device']:.1f} x; "
          f"device counts {r['device_counts']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
