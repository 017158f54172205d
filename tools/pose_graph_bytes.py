"""Prints a sha256 of every output of the pose-graph units (csrc/pgo.hip, csrc/loop_correct.hip) on fixed inputs, and writes them to --out as JSON.
Every sum in these units runs in a fixed order, so two builds that compute the same thing print the same listing: run it from two checkouts on one
GPU box and compare (profiles/pose_graph_pieces_bytes.json holds such a pair).  The inputs are those of the tests, taken from the test modules:
  pose_graph_optimize   synth.pose_graph(60, 1, seed=1) and (200, 2, seed=2) at 20 iterations; the mutated 120-key-frame graph of
                        test_pose_graph_general_structure; the 290-key-frame skip-2 graph (general Schur path) at 2 iterations; an all-fixed graph;
                        a graph with no edges
  correct_map_points    the 4 999 points of test_correct_map_points_device_on_a_caller_stream
  loop_local_fusion     the inputs of test_loop_local_fusion
  correct_batch         the mixed batch of tests/test_gpu_loop_correct.py: poses, points, edges, chi2, iterations, status
There is no pass / fail here: the tool reports."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (must precede the HIP library)
from __graft_entry__ import load_package  # noqa: E402
import pyoracle  # noqa: E402
import loop_correct_ref as R  # noqa: E402
import test_gpu_loop_correct as TL  # noqa: E402
import test_gpu_pgo as TP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
pkg = load_package(); api, synth = pkg.api, pkg.synth
oracle = pyoracle.Oracle()
out = {}


def note(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    out[name] = h.hexdigest()
    print(f"{name:44s} {out[name]}", flush=True)


def pgo(name, G, iters=20):
    poses, chi2, its = api.pose_graph_optimize(*G[:5], iters=iters)
    note(name, poses, np.float64(chi2), np.int32(its))


def general_structure_graph():
    """test_pose_graph_general_structure's graph: edges flipped, one duplicated, a second loop into the last loop's key-frame, two more fixed"""
    poses, fixed, e0, e1, meas, _ = synth.pose_graph(120, 3, seed=6)
    rng = np.random.default_rng(0)
    flip = rng.uniform(size=len(e0)) < 0.4
    inv = np.stack([oracle.se3_compose(np.array([0, 0, 0, 1, 0, 0, 0.0]), m, invert_b=True) for m in meas])
    e0f = np.where(flip, e1, e0); e1f = np.where(flip, e0, e1); mf = np.where(flip[:, None], inv, meas)
    e0f = np.concatenate([e0f, e0f[10:11], [e0f[-1] - 3]]); e1f = np.concatenate([e1f, e1f[10:11], [e1f[-1]]])
    extra = oracle.se3_compose(poses[e0f[-1]], poses[e1f[-1]], invert_b=True)
    mf = np.concatenate([mf, mf[10:11], extra[None]])
    fixed = fixed.copy(); fixed[40] = 1; fixed[41] = 1
    return poses, fixed, e0f.astype(np.int32), e1f.astype(np.int32), mf


pgo("pgo 60 key-frames, 1 loop", synth.pose_graph(60, 1, seed=1))
pgo("pgo 200 key-frames, 2 loops", synth.pose_graph(200, 2, seed=2))
pgo("pgo general structure, 120 key-frames", general_structure_graph())
pgo("pgo skip-2, 290 key-frames, general path", TP._skip2_graph(synth, oracle, 290), iters=2)
poses, fixed, e0, e1, meas, _ = synth.pose_graph(50, 1, seed=5)
pgo("pgo all fixed", (poses, np.ones_like(fixed), e0, e1, meas))
pgo("pgo no edges", (poses, fixed, e0[:0], e1[:0], meas[:0]))

poses, fixed, e0, e1, meas, _ = synth.pose_graph(80, 1, seed=8)
new = oracle.pose_graph_optimize(poses, fixed, e0, e1, meas)[0]
rng = np.random.default_rng(2)
kf = rng.integers(-3, 80, 4999).astype(np.int32); kf[:3] = [0, 79, -1]
note("correct_map_points, 4999 points", api.correct_map_points(poses, new, kf, rng.normal(0, 30, (4999, 3))))

rng = np.random.default_rng(5)
poses = synth.pose_graph(40, 1, seed=9)[0][-7:].copy()
corrected = oracle.se3_compose(poses[6], oracle.se3_exp(np.array([0.3, -0.1, 0.2, 0.02, -0.01, 0.03])))
pts = rng.uniform(-5, 5, (500, 3)) + np.array([0, 0, 15.0])
first = rng.integers(-1, 7, 500).astype(np.int32)
gp, gx = api.loop_local_fusion(poses, 6, corrected, first, pts)
note("loop_local_fusion poses", gp); note("loop_local_fusion points", gx)

make = {("needed", 60): (60, 1, 1, {}), ("needed", 120): (120, 2, 2, {}), ("needed", 200): (200, 3, 3, {}), ("needed", 30): (30, 1, 4, {}),
        ("small", 60): (60, 1, 5, dict(needed=False)), ("all-fixed", 11): (11, 0, 6, {}), ("one", 1): (1, 0, 7, dict(n_points=5))}
make.update({("skipped", vs): (30, 1, 10 + vs, dict(verify_status=vs)) for vs in (1, 2, 3)})
items = {k: R.build_item(synth, oracle, n, loops, seed, **kw) for k, (n, loops, seed, kw) in make.items()}
_, res = TL.run(api, [items[k] for k in TL.MIXED])
for key in ("poses", "points", "e0", "e1", "meas", "n_edges", "chi2", "iters", "status"):
    note("correct_batch " + key, res[key])
print("correct_batch status", res["status"].tolist(), "iterations", res["iters"].tolist())
out["build"] = api.build_id()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
