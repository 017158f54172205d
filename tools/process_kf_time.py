"""Times the ORB half of LoopClosing::ProcessNewKF for 16 key-frames x 200 features at 1241 x 376 on the GPU box:
  A  one ORBextractor.process_keyframes_batch on device buffers, eager and replayed from a StepGraph;
  B  the path of the commit before that call existed, per key-frame through the host: api.expand_pyramid_keypoints,
     ORBextractor.ScreenAndComputeKPsParams, ORBextractor.CalcDescriptors (two image uploads, two pyramids and two synchronisations each).

Host clock around calls that end in a stream synchronise; every form is warmed up, then timed in alternating rounds (A B A B ...) of REPS calls
each; medians with min - max go to profiles/process_kf_time.json (--out names another file).  There is no pass / fail ratio: the tool reports.

    python tools/process_kf_time.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "process_kf_time.json"))
opt = ap.parse_args()

pkg = load_package(); api, synth = pkg.api, pkg.synth
assert api.device_count() >= 1, "needs a HIP device: nothing here is measured on a CPU"
B, N, H, W, LEVELS, ROUNDS, REPS = 16, 200, 376, 1241, 8, 7, 10
CAP = N * LEVELS

imgs = np.stack([synth.stereo_pair(0, t)[0] for t in range(B)])
assert imgs.shape == (B, H, W) and imgs.dtype == np.uint8
stream = torch.cuda.Stream(); S = stream.cuda_stream
ext = api.ORBextractor(N, stream=S)                      # the call under test
old = api.ORBextractor(N, stream=S)                      # the per-key-frame path keeps a handle of its own, as chain.py's backend does
xy = np.full((B, N, 2), np.nan, np.float32); n_feat = np.zeros(B, np.int32)
for b in range(B):                                       # the frontend's features: level-0 corners of the key-frame's image
    k = old.Detect(imgs[b])[:N]
    n_feat[b] = len(k); xy[b, :len(k), 0] = k["x"]; xy[b, :len(k), 1] = k["y"]

with torch.cuda.stream(stream):
    d_imgs = torch.from_numpy(imgs).cuda(); d_xy = torch.from_numpy(xy).cuda(); d_n = torch.from_numpy(n_feat).cuda()
    d_kps = torch.zeros(B, CAP * 28, dtype=torch.uint8, device="cuda"); d_desc = torch.zeros(B, CAP, 32, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(B, dtype=torch.int32, device="cuda"); d_st = torch.zeros(B, dtype=torch.int32, device="cuda")


def new():
    ext.process_keyframes_batch(d_imgs.data_ptr(), B, H, W, W, H * W, d_xy.data_ptr(), d_n.data_ptr(), N, d_kps.data_ptr(), d_desc.data_ptr(),
                                d_cnt.data_ptr(), d_st.data_ptr(), CAP)


def previous():
    """chain.process_new_kf's ORB half, key-frame by key-frame: every call ends in a synchronisation of its own"""
    out = []
    for b in range(B):
        feats = np.zeros(n_feat[b], api.KP_DTYPE)
        feats["x"], feats["y"] = xy[b, :n_feat[b], 0], xy[b, :n_feat[b], 1]
        feats["size"], feats["angle"], feats["octave"], feats["class_id"] = 7, -1, 0, -1
        pyr, _ = old.ScreenAndComputeKPsParams(imgs[b], api.expand_pyramid_keypoints(feats, LEVELS))
        out.append((pyr, old.CalcDescriptors(imgs[b], pyr)))
    return out


def timed(fn):
    t = time.perf_counter()
    for _ in range(REPS):
        fn()
        stream.synchronize()
    return (time.perf_counter() - t) / REPS * 1e3


ref = previous()
new(); stream.synchronize()
cnt, st = d_cnt.cpu().numpy(), d_st.cpu().numpy()
kps, desc = d_kps.cpu().numpy(), d_desc.cpu().numpy()
same = all(st[b] == 0 and cnt[b] == len(ref[b][0]) and kps[b, :cnt[b] * 28].tobytes() == ref[b][0].tobytes() and np.array_equal(desc[b, :cnt[b]], ref[b][1])
           for b in range(B))
print(f"features {n_feat.tolist()}; pyramid key-points kept {cnt.tolist()}; the batch call equals the per-key-frame path bit for bit: {same}", flush=True)
assert same
graph = api.StepGraph.record(S, [], new)
forms = {"A process_keyframes_batch, eager": new, "A replayed from a StepGraph": lambda: graph.launch(S), "B per key-frame through the host": previous}
for fn in forms.values():                                # warm-up of every form
    timed(fn)
times = {k: [] for k in forms}
for _ in range(ROUNDS):                                  # A B A B ...
    for k, fn in forms.items():
        times[k].append(timed(fn))
res = {"workload": f"{B} key-frames x {N} features at {W} x {H}, {LEVELS} levels", "features": n_feat.tolist(), "kept": cnt.tolist(), "graph_nodes": graph.node_count(),
       "rounds": ROUNDS, "calls_per_round": REPS, "unit": "ms per call (all key-frames), host clock around enqueue + stream synchronise",
       "forms": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
       "equal_bit_for_bit": bool(same), "clock_mhz": float(api.shader_clock_mhz(S)), "build_id": api.build_id()}
for k, v in res["forms"].items():
    print(f"{k:36s} median {v['median']:8.3f} ms per {B} key-frames   (min {v['min']:.3f}, max {v['max']:.3f}, {ROUNDS} rounds x {REPS} calls)", flush=True)
print(f"graph nodes {res['graph_nodes']}, clock {res['clock_mhz']:.0f} MHz, build {res['build_id']}")
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
