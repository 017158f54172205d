"""Times the three link-upkeep launches at a batch of 64 (--batch): LoopKeyFrameStore.clear_links_batch (64 lists of 40 entries on the stride of the back
end's observation cap, half of them naming one of 64 stored key-frames of 512 features, a quarter the pending key-frame, a quarter a key-frame that
is not held), MapArchive.filter_landmarks_batch (64 gathered rows of 512 entries against archives of 30 000 map points, a tenth of them erased) and
Tracker.clear_links_batch (64 streams of 376 x 1241 right after their key-frame, 400 features, the same lists).

One such call is shorter than the host's cost of enqueuing it, so each is timed as a burst of 50 calls in one span and reported per call.  The writes
are idempotent: every clear of a burst does the same work; the gathered rows are put back before every burst, so its first filter drops and the
others read the whole rows and find nothing.  Host clock around spans that end in a synchronise; warmed up, then timed 25 times each in
alternation; medians with min - max go to profiles/link_upkeep_launches.json (--out names another file).  There is no pass / fail ratio: the tool reports."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_upkeep_launches.json"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api = pkg.api
B, BURST = args.batch, 50
LIST_CAP, N_LIST, KFS, FEAT_CAP, POINT_CAP, N_POINTS = 1987, 40, 64, 512, 32768, 30000
ROWS, COLS, N_FEAT = 376, 1241, 400
rng = np.random.default_rng(0x11AB)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
p = lambda t: t.data_ptr()

# ---- the loop store: KFS key-frames (ids 10, 12, ...), every link set
store = api.LoopKeyFrameStore(KFS + 1, 8, FEAT_CAP, stream=sp)
kf_ids = 10 + 2 * np.arange(KFS)
d_kps = torch.zeros((KFS, 8, 28), dtype=torch.uint8, device="cuda"); d_desc = torch.zeros((KFS, 8, 32), dtype=torch.uint8, device="cuda")
d_cnt = torch.zeros(KFS, dtype=torch.int32, device="cuda"); d_nf = torch.full((KFS,), FEAT_CAP, dtype=torch.int32, device="cuda")
d_lm = torch.from_numpy(rng.integers(0, N_POINTS, (KFS, FEAT_CAP)).astype(np.int32)).cuda()
torch.cuda.synchronize()
store.put_batch(kf_ids, p(d_kps), p(d_desc), p(d_cnt), 0, p(d_lm), p(d_nf))
pending_id = int(kf_ids[-1]) + 2
ids = np.full((B, LIST_CAP), -1, np.int64); tags = np.full((B, LIST_CAP), -1, np.int32)
kind = rng.integers(0, 4, (B, N_LIST))
ids[:, :N_LIST] = np.where(kind < 2, rng.choice(kf_ids, (B, N_LIST)), np.where(kind == 2, pending_id, 11))
tags[:, :N_LIST] = rng.integers(0, N_FEAT, (B, N_LIST))
d_ids, d_tags = torch.from_numpy(ids).cuda(), torch.from_numpy(tags).cuda()
d_n = torch.full((B,), N_LIST, dtype=torch.int32, device="cuda")
d_pid = torch.full((B,), pending_id, dtype=torch.int64, device="cuda")
d_pend = torch.from_numpy(rng.integers(0, N_POINTS, (B, FEAT_CAP)).astype(np.int32)).cuda()
d_cleared = torch.zeros(B, dtype=torch.int32, device="cuda")

# ---- the archive: N_POINTS map points per stream, a tenth erased; the gathered rows name any of them
arc = api.MapArchive(B, 2, 2, POINT_CAP, 8, stream=sp)
state = (rng.random(N_POINTS) < 0.1).astype(np.uint8) * 2
for b in range(B):
    arc.load(b, [1], [(0, 0, 0, 1, 0, 0, 0)], [], [], np.zeros((0, 7)), np.arange(N_POINTS), np.zeros((N_POINTS, 3)), np.full(N_POINTS, -1, np.int32), state)
rows = rng.integers(-1, N_POINTS, (B, FEAT_CAP)).astype(np.int32)
d_rows = torch.from_numpy(rows).cuda(); d_rows0 = d_rows.clone()
d_dropped = torch.zeros(B, dtype=torch.int32, device="cuda")

# ---- the tracker: B streams whose last frame is their reference key-frame's frame
K = (718.856, 718.856, 607.1928, 185.2157)
trk = api.Tracker(B, ROWS, COLS, 512, 1024, K, stream=sp)
img = rng.integers(0, 256, (ROWS, COLS)).astype(np.uint8)
st = dict(xy=rng.uniform(20, 300, (N_FEAT, 2)).astype(np.float32), lm=np.arange(N_FEAT, dtype=np.int32), lm_pos=rng.uniform(5, 30, (N_FEAT, 3)),
          lm_outlier=np.zeros(N_FEAT, np.uint8), ref_pose=np.array([0, 0, 0, 1, 0, 0, 0.0]), ref_frame_id=4, last_rel=np.eye(4), rel_motion=np.eye(4),
          next_frame_id=5, status=1, kf_every=0)
for s in range(B):
    trk.set_frame(s, st, image=img)
    trk.set_ids(s, 100 + np.arange(N_FEAT), pending_id, pending_id + 1, 100 + N_FEAT)
d_tcleared = torch.zeros(B, dtype=torch.int32, device="cuda")


def burst(body, before=None):
    def f():
        with torch.cuda.stream(stream):
            if before:
                before()
        for _ in range(BURST):
            body()
    return f


forms = {"loop_store clear_links_batch": burst(lambda: store.clear_links_batch(p(d_ids), p(d_tags), p(d_n), LIST_CAP, B, p(d_pid), p(d_pend), p(d_cleared))),
         "map filter_landmarks_batch": burst(lambda: arc.filter_landmarks_batch(p(d_rows), FEAT_CAP, B, p(d_dropped)), lambda: d_rows.copy_(d_rows0)),
         "tracker clear_links_batch": burst(lambda: trk.clear_links_batch(p(d_ids), p(d_tags), p(d_n), LIST_CAP, p(d_tcleared)))}
ms = {k: [] for k in forms}
stream.wait_stream(torch.cuda.current_stream())
for f in forms.values():
    f(); torch.cuda.synchronize()
counts = dict(cleared=int(d_cleared.sum()), tracker_cleared=int(d_tcleared.sum()))
d_rows.copy_(d_rows0); torch.cuda.synchronize()                             # (the rows are restored before every burst: its first call drops, the others find nothing)
arc.filter_landmarks_batch(p(d_rows), FEAT_CAP, B, p(d_dropped)); torch.cuda.synchronize()
counts["dropped"] = int(d_dropped.sum())
for _ in range(args.reps):
    for k, f in forms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / BURST)
res = {"workload": f"batch {B}: lists of {N_LIST} entries on a stride of {LIST_CAP}, {KFS} stored key-frames x {FEAT_CAP} features; rows of {FEAT_CAP} entries against "
                   f"{N_POINTS} map points per stream; {B} streams of {ROWS} x {COLS} with {N_FEAT} features", "calls_per_burst": BURST, "bursts": args.reps,
       "counts": counts, "ms_per_call": {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}}
for k, v in res["ms_per_call"].items():
    print(f"{k:34s} median {v['median'] * 1e3:8.2f} us per call   (min {v['min'] * 1e3:.2f}, max {v['max'] * 1e3:.2f}; bursts of {BURST}, {args.reps} bursts)", flush=True)
res["clock_mhz"] = float(api.shader_clock_mhz(sp)); res["build"] = api.build_id()
print(f"counts {counts}, clock {res['clock_mhz']:.0f} MHz, build {res['build']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
