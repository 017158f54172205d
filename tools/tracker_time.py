"""Per-frame tracking of S camera streams, two ways on one device, alternating A B A B:
  A  the one-camera way, S times per frame: myslam_lk_track_cached + myslam_pose_only_optimize with the host glue of chain.track() between
     them (re-projection of the landmarks, feature filtering, SE3 bookkeeping; the glue is vectorised numpy here, which favours A over chain.py's
     per-feature loops);
  B  one myslam_tracker_step_batch for all streams + one download of the S result records.
S = 1, 8, 64, 256 at 1241 x 376 with ~150 and ~400 tracked features per stream; >= 200 steps after warm-up; median and p90 per step, wall clock
and HIP events (B only: A synchronises inside every call, its device time is not separable from the host's).  Both ways track the same image
pair from the same states; in steady state the camera stands still (frame t + 1 = frame t), so that every step does the same work.
Writes profiles/tracker_time.json.

    python tools/tracker_time.py [--steps 200] [--out profiles/tracker_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one HIP runtime for the process: before the library)

from __graft_entry__ import load_package  # noqa: E402

ROWS, COLS = 376, 1241


def make_stream(pkg, n_feat, seed):
    """an image, n_feat corners of it with landmarks at random depths seen from the identity pose"""
    api, synth = pkg.api, pkg.synth
    img = synth.random_image(seed, ROWS, COLS)
    kp = api.ORBextractor(4 * n_feat).Detect(img)
    ok = (kp["x"] > 30) & (kp["x"] < COLS - 30) & (kp["y"] > 30) & (kp["y"] < ROWS - 30)
    kp = kp[ok][:n_feat]
    K = synth.KITTI00
    z = np.random.default_rng(seed).uniform(5, 40, len(kp))
    pos = np.stack([(kp["x"] - K["cx"]) * z / K["fx"], (kp["y"] - K["cy"]) * z / K["fy"], z], 1).astype(np.float64)
    st = {"xy": np.stack([kp["x"], kp["y"]], 1).astype(np.float32), "lm": np.arange(len(kp), dtype=np.int32), "lm_pos": pos,
          "lm_outlier": np.zeros(len(kp), np.uint8), "ref_pose": np.array([0, 0, 0, 1, 0, 0, 0.0]), "ref_frame_id": 0, "last_rel": np.eye(4),
          "rel_motion": np.eye(4), "next_frame_id": 1, "status": 1, "kf_every": 0}
    return img, st


class OneCamera:
    """way A for one stream: chain.track() up to the key-frame branch on arrays"""
    def __init__(self, pkg, img, st, Kt):
        self.api, self.chain, self.Kt = pkg.api, pkg.chain, Kt
        self.lk = pkg.api.LKTracker()
        self.img, self.tok = img, 1
        self.xy, self.pos = st["xy"].copy(), st["lm_pos"].copy()
        self.Tref = self.chain.T_of(st["ref_pose"]); self.Tref_inv = self.chain.T_inv(self.Tref)
        self.rel, self.motion = np.eye(4), np.eye(4)

    def frame(self, img, tok):
        ch = self.chain
        rel = ch.mm(self.motion, self.rel)
        Tcw = ch.mm(rel, self.Tref)
        pc = self.pos @ Tcw[:3, :3].T + Tcw[:3, 3]
        p1 = np.stack([self.Kt[0] * pc[:, 0] / pc[:, 2] + self.Kt[2], self.Kt[1] * pc[:, 1] / pc[:, 2] + self.Kt[3]], 1).astype(np.float32)
        nxt, st, _ = self.lk.track_cached(self.img, self.tok, img, tok, self.xy, p1)
        xy, pos = nxt[st], self.pos[st]
        pose, outl, n_inl = self.api.pose_only_optimize(ch.p7_of(Tcw), pos, xy.astype(np.float64), self.Kt)
        new = ch.mm(ch.T_of(pose), self.Tref_inv)
        self.motion = ch.mm(new, ch.T_inv(self.rel)); self.rel = new
        self.xy, self.pos = xy[~outl], pos[~outl]
        self.img, self.tok = img, tok
        return n_inl


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(ms)), "p90_ms": float(ms[int(0.9 * (len(ms) - 1))]), "steps": len(ms)}


def run_a(pkg, streams, Kt, steps, warm):
    cams = [OneCamera(pkg, img, st, Kt) for img, st in streams]
    out = []
    for k in range(warm + steps):
        t0 = time.perf_counter()
        n = [c.frame(streams[i][0], 2) for i, c in enumerate(cams)]
        if k >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return stats(out), int(np.median(n))


def run_b(pkg, streams, Kt, steps, warm):
    api = pkg.api
    S = len(streams)
    nmax = max(len(st["xy"]) for _, st in streams)
    cap = 256 if nmax <= 256 else 512
    trk = api.Tracker(S, ROWS, COLS, cap, cap, Kt, 50, 10)
    for s, (img, st) in enumerate(streams):
        trk.set_frame(s, st, image=img)
    d_img = torch.from_numpy(np.stack([img for img, _ in streams])).cuda()
    d_res = torch.zeros(S * 80, dtype=torch.uint8, device="cuda")
    h_res = torch.zeros(S * 80, dtype=torch.uint8).pin_memory()
    wall, dev = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warm + steps):
        t0 = time.perf_counter()
        e0.record()
        trk.step_batch(d_img.data_ptr(), COLS, ROWS * COLS, d_res.data_ptr())
        e1.record()
        h_res.copy_(d_res)                                # the one download of the step (synchronises)
        if k >= warm:
            wall.append((time.perf_counter() - t0) * 1e3); dev.append(e0.elapsed_time(e1))
    r = h_res.numpy().view(api.TRACKER_RESULT_DTYPE)
    assert (r["needs_host"] == 0).all() and (r["frame_id"] == warm + steps).all(), "a stream froze: the timed steps did not all do their work"
    return stats(wall), stats(dev), int(np.median(r["n_inliers"])), trk.launches_per_step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_time.json"))
    a = ap.parse_args()
    pkg = load_package()
    K = pkg.synth.KITTI00
    Kt = (K["fx"], K["fy"], K["cx"], K["cy"])
    base = {n: [make_stream(pkg, n, 100 + i) for i in range(8)] for n in (150, 400)}
    rows = []
    for n_feat in (150, 400):
        for S in a.streams:
            streams = [base[n_feat][i % 8] for i in range(S)]
            A, B = [], []
            for _ in range(2):                            # A B A B
                A.append(run_a(pkg, streams, Kt, a.steps, a.warmup))
                B.append(run_b(pkg, streams, Kt, a.steps, a.warmup))
            fa = [1e3 * S / x[0]["median_ms"] for x in A]; fb = [1e3 * S / x[0]["median_ms"] for x in B]
            row = {"streams": S, "features": n_feat, "inliers_A": A[0][1], "inliers_B": B[0][2], "launches_per_step_B": B[0][3],
                   "A_wall": [x[0] for x in A], "B_wall": [x[0] for x in B], "B_hip_events": [x[1] for x in B],
                   "A_frames_per_s": fa, "B_frames_per_s": fb, "A_spread": abs(fa[0] - fa[1]) / min(fa),
                   "B_over_A": min(fb) / max(fa)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/tracker_time.py", "image": [ROWS, COLS], "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
                   "rows": rows}, f, indent=1)
    for r in rows:
        if r["streams"] >= 8:
            assert r["B_over_A"] > 1.0 + r["A_spread"], f"B does not beat A beyond A's own spread at S = {r['streams']}, {r['features']} features: {r}"


if __name__ == "__main__":
    main()
