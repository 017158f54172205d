"""Times loop correction of 16 maps x 200 key-frames x 2 loops x 5 000 points on the GPU box: one LoopCorrector.correct_batch (device tables, one
enqueue) against the per-map path on the same items, 16 x (api.loop_local_fusion + api.pose_graph_optimize + api.correct_map_points) through host
pointers.

Host clock around calls that end in a device synchronise (the one-map calls synchronise themselves); the batch form restores its in/out tables by
device-to-device copies on its stream before every call, inside the timed span.  Both forms are warmed up, then timed 20 times each in alternation;
medians with min - max go to profiles/loop_correct_time.json (--out names another file).  The batch form is also timed with max_iters = 0 and 1
(everything but the Levenberg iterations, and one of them), which splits its time into phases.  There is no pass / fail ratio: the tool reports."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_correct_time.json"))
args = ap.parse_args()
pkg = load_package(); api, synth = pkg.api, pkg.synth
B, N, LOOPS, NPTS, NACT, REPS = 16, 200, 2, 5000, 10, 20


def T_of(p):
    T = np.eye(4); T[:3, :3] = synth._quat_to_R(p[:4] / np.linalg.norm(p[:4])); T[:3, 3] = p[4:]
    return T


def make_item(seed):
    """synth's drive with its last loop edge taken off (the call appends it), the active window moved by a rigid motion of ~1.7 m"""
    poses, _, e0, e1, meas, _ = synth.pose_graph(N, LOOPS, seed=seed, n_active=NACT)
    cur, loop = int(e0[-1]), int(e1[-1])
    assert cur == N - 1
    corrected = synth._T_to_pose7(T_of(meas[-1]) @ T_of(poses[loop]))
    D = np.eye(4); D[:3, 3] = [1.5, -0.4, 0.8]
    active = np.arange(N - NACT, N, dtype=np.int32)
    poses = poses.copy()
    for a in active:
        poses[a] = synth._T_to_pose7(T_of(poses[a]) @ D)
    rng = np.random.default_rng(seed)
    fa = np.where(rng.uniform(size=NPTS) < 0.2, rng.integers(0, NACT, NPTS), -1).astype(np.int32)
    fk = np.where(fa >= 0, active[np.maximum(fa, 0)], rng.integers(0, N, NPTS)).astype(np.int32)
    return dict(poses=poses, active=active, cur=cur, loop=loop, corrected=corrected, e0=e0[:-1].copy(), e1=e1[:-1].copy(), meas=meas[:-1].copy(),
                points=rng.normal(0, 30, (NPTS, 3)), fa=fa, fk=fk)


items = [make_item(100 + s) for s in range(B)]
E = len(items[0]["e0"]); ECAP = E + 1
stream = torch.cuda.Stream()
lc = api.LoopCorrector(B, N, ECAP, NACT, NPTS, stream=stream.cuda_stream)


def table(key, dtype, shape):
    out = np.zeros((B,) + shape, dtype)
    for b, it in enumerate(items):
        v = np.asarray(it[key], dtype)
        out[(b,) + tuple(slice(0, s) for s in v.shape)] = v
    return out


host = dict(poses=table("poses", np.float64, (N, 7)), active=table("active", np.int32, (NACT,)), corrected=table("corrected", np.float64, (7,)),
            e0=table("e0", np.int32, (ECAP,)), e1=table("e1", np.int32, (ECAP,)), meas=table("meas", np.float64, (ECAP, 7)),
            points=table("points", np.float64, (NPTS, 3)), fa=table("fa", np.int32, (NPTS,)), fk=table("fk", np.int32, (NPTS,)),
            n_kf=np.full(B, N, np.int32), n_active=np.full(B, NACT, np.int32), cur=np.array([it["cur"] for it in items], np.int32),
            loop=np.array([it["loop"] for it in items], np.int32), n_edges=np.full(B, E, np.int32), n_points=np.full(B, NPTS, np.int32))
with torch.cuda.stream(stream):
    d = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    keep = {k: d[k].clone() for k in ("poses", "points", "n_edges")}
    chi2 = torch.zeros(B, dtype=torch.float64, device="cuda"); iters = torch.zeros(B, dtype=torch.int32, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")


def batch(max_iters=20):
    with torch.cuda.stream(stream):
        for k, v in keep.items():
            d[k].copy_(v)
    lc.correct_batch(d["poses"].data_ptr(), d["n_kf"].data_ptr(), d["active"].data_ptr(), d["n_active"].data_ptr(), d["cur"].data_ptr(), d["loop"].data_ptr(),
                     d["corrected"].data_ptr(), 0, d["e0"].data_ptr(), d["e1"].data_ptr(), d["meas"].data_ptr(), d["n_edges"].data_ptr(), d["points"].data_ptr(),
                     d["n_points"].data_ptr(), d["fa"].data_ptr(), d["fk"].data_ptr(), B, 1.0, max_iters, chi2.data_ptr(), iters.data_ptr(), status.data_ptr())


def per_map():
    out = []
    for it in items:
        act = it["active"]
        fa_poses, pts = api.loop_local_fusion(it["poses"][act], int(np.where(act == it["cur"])[0][0]), it["corrected"], it["fa"], it["points"])
        fused = it["poses"].copy(); fused[act] = fa_poses
        Tm = T_of(it["corrected"]) @ np.linalg.inv(T_of(it["poses"][it["loop"]]))
        e0 = np.r_[it["e0"], it["cur"]].astype(np.int32); e1 = np.r_[it["e1"], it["loop"]].astype(np.int32)
        meas = np.concatenate([it["meas"], synth._T_to_pose7(Tm)[None]])
        fixed = np.zeros(N, np.uint8); fixed[act] = 1; fixed[it["loop"]] = 1; fixed[0] = 1
        opt, c, n_it = api.pose_graph_optimize(fused, fixed, e0, e1, meas)
        pts = api.correct_map_points(fused, opt, np.where(it["fa"] < 0, it["fk"], -1).astype(np.int32), pts)
        out.append((opt, pts, c, n_it))
    return out


def timed(fn, sync):
    t = time.perf_counter()
    fn()
    if sync:
        stream.synchronize()
    return (time.perf_counter() - t) * 1e3


batch(); stream.synchronize(); ref = per_map()
gp, gx, gc, gi, gs = (x.cpu().numpy() for x in (d["poses"], d["points"], chi2, iters, status))
pose_diff = max(np.abs(gp[b] - ref[b][0]).max() for b in range(B)); point_diff = max(np.abs(gx[b] - ref[b][1]).max() for b in range(B))
chi_diff = max(abs(gc[b] - ref[b][2]) / ref[b][2] for b in range(B))
print(f"results: status {gs.tolist()}; iterations batch {gi.tolist()} per-map {[r[3] for r in ref]}; largest pose difference {pose_diff:.2e}, "
      f"point difference {point_diff:.2e}, chi2 relative {chi_diff:.2e}", flush=True)
forms = {"correct_batch": (batch, True), "correct_batch, max_iters 0": (lambda: batch(0), True), "correct_batch, max_iters 1": (lambda: batch(1), True),
         "16 x per-map calls": (per_map, False)}
for fn, sync in forms.values():                      # warm-up of every form
    for _ in range(2):
        timed(fn, sync)
times = {k: [] for k in forms}
for _ in range(REPS):
    for k, (fn, sync) in forms.items():
        times[k].append(timed(fn, sync))
res = {"workload": f"{B} maps x {N} key-frames x {LOOPS} loops x {NPTS} points, {NACT} active key-frames, max_iters 20", "status": gs.tolist(),
       "iterations_batch": gi.tolist(), "iterations_per_map": [int(r[3]) for r in ref], "largest_pose_difference": float(pose_diff),
       "largest_point_difference": float(point_diff), "largest_chi2_relative_difference": float(chi_diff), "calls_per_form": REPS, "ms": {}}
for k, v in times.items():
    res["ms"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(f"{k:28s} median {np.median(v):9.3f} ms per {B} maps   (min {min(v):.3f}, max {max(v):.3f}, {REPS} calls)", flush=True)
res["clock_mhz"] = float(api.shader_clock_mhz(stream.cuda_stream)); res["build"] = api.build_id()
print(f"clock {res['clock_mhz']:.0f} MHz, build {res['build']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
