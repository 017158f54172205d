"""Times loop verification of 16 candidates x 200 matches on the GPU box: one PnPSolver.verify_batch (device buffers, one enqueue) against what the
one-item calls offer, 16 x (api.solve_pnp_ransac + api.pose_only_optimize(pre_optimize=1)) through host pointers.

Host clock around calls that end in a device synchronise (the one-item calls synchronise themselves); both forms are warmed up, then timed in
alternating rounds of REPS calls each, and the median round is reported together with the spread.  The batch form is also timed per stage
(solve_batch alone) and as a replayed StepGraph."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package(); api, synth = pkg.api, pkg.synth
B, N, ROUNDS, REPS = 16, 200, 7, 20

items = [synth.pnp_problem(N, 0.3, 0.5, seed=s) for s in range(B)]
K = items[0][2]
p3 = np.stack([it[0] for it in items]); p2 = np.stack([it[1] for it in items]); cnt = np.full(B, N, np.int32)
stream = torch.cuda.Stream()
solver = api.PnPSolver(B, N, 100, stream=stream.cuda_stream)
with torch.cuda.stream(stream):
    d_p3, d_p2, d_cnt = (torch.from_numpy(x).cuda() for x in (p3, p2, cnt))
    pose = torch.zeros(B, 7, dtype=torch.float64, device="cuda"); flag = torch.zeros(B, N, dtype=torch.uint8, device="cuda")
    ninl = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.zeros(B, dtype=torch.int32, device="cuda")


def batch():
    solver.verify_batch(d_p3.data_ptr(), d_p2.data_ptr(), d_cnt.data_ptr(), B, K, pose.data_ptr(), flag.data_ptr(), ninl.data_ptr(), st.data_ptr())


def batch_pnp_only():
    solver.solve_batch(d_p3.data_ptr(), d_p2.data_ptr(), d_cnt.data_ptr(), B, K, pose.data_ptr(), flag.data_ptr(), ninl.data_ptr(), st.data_ptr())


def single():
    out = []
    for pw, uv, _, _, _ in items:
        g = api.solve_pnp_ransac(pw, uv, K)
        out.append(api.pose_only_optimize(g[0], pw.astype(np.float64), uv.astype(np.float64), K, pre_optimize=1))
    return out


def timed(fn, sync):
    t = time.perf_counter()
    for _ in range(REPS):
        fn()
        if sync:
            stream.synchronize()
    return (time.perf_counter() - t) / REPS * 1e3


batch(); stream.synchronize(); ref = single()
gp = pose.cpu().numpy(); gn = ninl.cpu().numpy()
worst = max(np.abs(gp[b] - ref[b][0]).max() for b in range(B))
print(f"results: inliers batch {gn.tolist()} one-item {[r[2] for r in ref]}; largest pose difference {worst:.2e}; status {st.cpu().numpy().tolist()}", flush=True)
graph = api.StepGraph.record(stream.cuda_stream, [], batch)
forms = {"verify_batch": (batch, True), "verify_batch replayed": (lambda: graph.launch(stream.cuda_stream), True), "solve_batch only": (batch_pnp_only, True),
         "16 x one-item calls": (single, False)}
for fn, sync in forms.values():                      # warm-up of every form
    timed(fn, sync)
times = {k: [] for k in forms}
for _ in range(ROUNDS):
    for k, (fn, sync) in forms.items():
        times[k].append(timed(fn, sync))
for k, v in times.items():
    print(f"{k:24s} median {np.median(v):8.3f} ms per {B} candidates   (min {min(v):.3f}, max {max(v):.3f}, {ROUNDS} rounds x {REPS} calls)", flush=True)
print(f"clock {api.shader_clock_mhz(stream.cuda_stream):.0f} MHz, build {api.build_id()}")
