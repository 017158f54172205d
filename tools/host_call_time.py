"""Host-clock medians (ms) of the synchronous host-pointer calls that stage through HostCall: pose graph, PnP-RANSAC, map-point correction and the host
BA forms, each after one warm-up call per shape (GPU box).  Prints one JSON line.

    python tools/host_call_time.py [path/to/libmyslam_hip.so]     # another build's library, e.g. the parent commit's, for an old-against-new run
"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (must precede the HIP library)
from __graft_entry__ import load_package
pkg = load_package(); api, synth = pkg.api, pkg.synth
if len(sys.argv) > 1:
    api.LIB_PATH = os.path.abspath(sys.argv[1])


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


T = {"build": api.build_id()}
for n, l, reps in ((200, 2, 7), (1500, 6, 5), (4500, 17, 5), (20000, 40, 3)):
    G = synth.pose_graph(n, l, seed=n)[:5]
    T[f"pgo_{n}:{l}"] = median_ms(lambda: api.pose_graph_optimize(*G), reps)
for n, frac in ((100, 0.3), (400, 0.5), (2000, 0.6)):
    pw, uv, K, _, _ = synth.pnp_problem(n, frac, 0.5, seed=n)
    T[f"pnp_{n}"] = median_ms(lambda: api.solve_pnp_ransac(pw, uv, K), 20)
G = synth.pose_graph(200, 2, seed=200)
rng = np.random.default_rng(1)
kf = rng.integers(-1, 200, 5000).astype(np.int32); pts = rng.normal(0, 30, (5000, 3))
T["correct_map_points_5000"] = median_ms(lambda: api.correct_map_points(G[0], G[5], kf, pts), 20)
ba = synth.ba_problem(seed=0xBA, n_kf=7, n_mp=300)
T["ba_optimize_active_map_host_7x300"] = median_ms(lambda: api.ba_optimize_active_map(*ba), 20)
T["ba_build_host_7x300"] = median_ms(lambda: api.ba_build(*ba), 20)
print(json.dumps(T), flush=True)
