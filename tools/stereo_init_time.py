"""Times StereoInit of the multi-stream tracker on the GPU box for 16 and 64 streams at 1241 x 376 with the key-points the init extractor finds
(ORBextractor(300), the configuration's ORBextractor.nInitFeatures):

  device   Tracker.init_masks -> ORBextractor.detect_batch -> Tracker.init_batch, three asynchronous calls on one stream, one synchronise;
  host     the same starts the way chain.StreamBank.advance takes them without device_init, in the same library: per stream Chain.grab's
           StereoInit on arrays (the three synchronous single-image calls ORBextractor.Detect, LKTracker.track, triangulate_stereo, the map
           points and the table built in Python) and StreamBank.hand_off (set_frame with the image + set_ids).

Before every timed call the streams are put back into the created state (reset_stream: not timed).  Host clock around spans that end in a
synchronise; both forms warmed up, then timed REPS times in alternation; medians with min - max go to profiles/stereo_init_time.json (--out
names another file).  There is no pass / fail ratio: the tool reports what it reads."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_init_time.json"))
ap.add_argument("--streams", type=int, nargs="+", default=[16, 64])
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api, chain, synth = pkg.api, pkg.chain, pkg.synth
ROWS, COLS, NINIT, INIT_GOOD, CAP, LM_CAP, D = 376, 1241, 300, 100, 512, 1024, 4
K = (718.856, 718.856, 607.1928, 185.2157); BASE = 0.537


def stream_case(seed):
    """a stream's first stereo pair: the right image = the left moved by D pixels"""
    big = synth.random_image(seed, ROWS + 16, COLS + 16, "texture")
    return np.ascontiguousarray(big[8:8 + ROWS, 8:8 + COLS]), np.ascontiguousarray(big[8:8 + ROWS, 8 + D:8 + D + COLS])


def host_init(trk, orb, lk, s, left, right):
    """one stream's start through the host: the steps of Chain.detect_features / find_features_in_right / build_init_map / insert_keyframe and
    StreamBank.hand_off on arrays"""
    mask = np.full((ROWS, COLS), 255, np.uint8)
    new = orb.Detect(left, mask)
    p0 = np.stack([new["x"], new["y"]], 1).astype(np.float32)
    nxt, ok, _ = lk.track(left, right, p0, p0.copy())
    if np.count_nonzero(ok) < INIT_GOOD:
        return len(new), int(np.count_nonzero(ok)), -1
    cand = [i for i in range(len(p0)) if ok[i]]
    xyz, tok = api.triangulate_stereo(p0[cand, 0], p0[cand, 1], nxt[cand, 0], nxt[cand, 1], *K, BASE) if cand else (np.zeros((0, 3)), np.zeros(0, bool))
    lm, pos = np.full(len(p0), -1, np.int32), []
    for j, i in enumerate(cand):
        if tok[j]:
            lm[i] = len(pos); pos.append(xyz[j])
    st = {"xy": p0, "lm": lm, "lm_pos": np.array(pos, float).reshape(-1, 3), "lm_outlier": np.zeros(len(pos), np.uint8), "ref_pose": chain.IDENT.copy(),
          "ref_frame_id": 0, "last_rel": np.eye(4), "rel_motion": np.eye(4), "next_frame_id": 1, "status": 1, "kf_every": 0}
    trk.set_frame(s, st, image=left)
    trk.set_ids(s, np.arange(len(pos), dtype=np.int64), 0, 1, len(pos))
    return len(new), int(np.count_nonzero(ok)), len(pos)


def measure(S):
    made = [stream_case(100 + s) for s in range(S)]
    stream = torch.cuda.Stream()
    trk = api.Tracker(S, ROWS, COLS, CAP, LM_CAP, K, stream=stream.cuda_stream)
    orb, lk = api.ORBextractor(NINIT, stream=stream.cuda_stream), api.LKTracker()
    kp_cap = int(orb.max_keypoints(ROWS, COLS))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    out = {"new_kf_id": z(S, torch.int64), "new_kf_pose": z((S, 7), torch.float64), "feat_mp_id": z((S, CAP), torch.int64), "feat_mp_pos": z((S, CAP, 3), torch.float64),
           "feat_uv": z((S, CAP, 2), torch.float32), "feat_tag": z((S, CAP), torch.int32), "feat_flags": z((S, CAP), torch.uint8), "n_feat": z(S, torch.int32),
           "outlier_mp_id": z((S, 2 * CAP), torch.int64), "n_outlier_mp": z(S, torch.int32), "right_xy": z((S, CAP, 2), torch.float32),
           "right_ok": z((S, CAP), torch.uint8), "report": z((S, 8), torch.int32)}
    d_left = torch.from_numpy(np.stack([m[0] for m in made])).cuda(); d_right = torch.from_numpy(np.stack([m[1] for m in made])).cuda()
    d_mask = z((S, ROWS, COLS), torch.uint8); d_kps = z((S, kp_cap, 28), torch.uint8); d_n = z(S, torch.int32); d_st = z(S, torch.int32)
    torch.cuda.synchronize()
    img = ROWS * COLS

    def reset():
        for s in range(S):
            trk.reset_stream(s)

    def device():
        trk.init_masks(d_mask.data_ptr(), COLS, img)
        orb.detect_batch(d_left.data_ptr(), S, ROWS, COLS, COLS, img, d_kps.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), kp_cap, d_masks=d_mask.data_ptr())
        trk.init_batch(d_left.data_ptr(), d_right.data_ptr(), COLS, img, d_kps.data_ptr(), d_n.data_ptr(), kp_cap, BASE, INIT_GOOD,
                       {k: v.data_ptr() for k, v in out.items()})
        stream.synchronize()

    def host():
        return [host_init(trk, orb, lk, s, made[s][0], made[s][1]) for s in range(S)]

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
    assert (hc[:, 0] == rep[:, 2]).all() and (hc[:, 1] == rep[:, 3]).all() and (hc[:, 2] == rep[:, 4]).all(), "the two forms did not do the same work"
    res = {"streams": S, "counts": {"detected": [int(rep[:, 2].min()), int(rep[:, 2].max())], "right_matches": [int(rep[:, 3].min()), int(rep[:, 3].max())],
                                    "map_points": [int(rep[:, 4].min()), int(rep[:, 4].max())]},
           "launches": {"masks": 1, "init": trk.init_launches()}, "ms": {}}
    for k, v in times.items():
        res["ms"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
        print(f"{S:3d} streams  {k:7s} median {np.median(v):10.3f} ms   (min {min(v):.3f}, max {max(v):.3f}, {args.reps} calls)", flush=True)
    res["host_over_device"] = res["ms"]["host"]["median"] / res["ms"]["device"]["median"]
    res["clock_mhz"] = float(api.shader_clock_mhz(stream.cuda_stream))
    return res


result = {"workload": f"{ROWS} x {COLS}, ORBextractor({NINIT}) over the whole image, initGood {INIT_GOOD}, cap {CAP}, landmark cap {LM_CAP}, disparity {D} px",
          "calls_per_form": args.reps, "runs": [measure(S) for S in args.streams], "build": api.build_id()}
for r in result["runs"]:
    print(f"{r['streams']} streams: host {r['ms']['host']['median']:.1f} ms, device {r['ms']['device']['median']:.2f} ms: {r['host_over_device']:.1f} x; "
          f"counts {r['counts']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
