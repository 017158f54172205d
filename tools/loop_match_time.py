"""Times the loop closer's chain from "the database names a loop key-frame" to the verdict for 16 candidates x 1 600 pyramid rows (200 features x 8
levels) on the GPU box: one api.loop_match_batch + PnPSolver.verify_batch on device buffers (eager, and replayed from a StepGraph) against the path
of the commit before loop_match_batch existed: api.hamming_match_batch, download of its output, api.match_feature_pairs and a numpy gather per
candidate, upload of the point arrays, verify_batch.

Host clock around calls that end in a stream synchronise; every form is warmed up, then timed in alternating rounds of REPS calls each, and the median
round is reported together with the spread.  The match stage alone is timed in both forms as well."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package(); api, synth = pkg.api, pkg.synth
B, N, LEVELS, ROUNDS, REPS = 16, 200, 8, 7, 20
CAP = N * LEVELS


def flipped(rows, nbits, rng):
    """each 256-bit row with nbits[i] random bits flipped"""
    order = np.argsort(rng.random((len(rows), 256)), axis=1)
    bits = np.zeros((len(rows), 256), np.uint8)
    np.put_along_axis(bits, order, (np.arange(256)[None, :] < nbits[:, None]).astype(np.uint8), axis=1)
    return rows ^ np.packbits(bits, axis=1, bitorder="little")


# every point of a synth.pnp_problem is a feature of both key-frames with LEVELS pyramid rows; every seventh loop feature has no map point
ld = np.zeros((B, CAP, 32), np.uint8); cd = np.zeros((B, CAP, 32), np.uint8)
lp = np.zeros((B, CAP), api.KP_DTYPE); cp = np.zeros((B, CAP), api.KP_DTYPE)
xy = np.zeros((B, N, 2), np.float32); lm = np.zeros((B, N), np.int32); pos = np.zeros((B, N, 3))
K = None
for b in range(B):
    pw, uv, K, _, _ = synth.pnp_problem(N, 0.3, 0.5, seed=b)
    rng = np.random.default_rng(1000 + b)
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    cls = np.repeat(np.arange(N), LEVELS); rows = rng.permutation(CAP)
    ld[b] = flipped(base[cls[rows]], rng.integers(0, 12, CAP), rng); lp["class_id"][b] = cls[rows]
    cd[b] = flipped(base[cls], rng.integers(0, 4, CAP), rng); cp["class_id"][b] = cls
    xy[b] = uv; lm[b] = np.where(np.arange(N) % 7 == 6, -1, np.arange(N)); pos[b] = pw
cnt_rows = np.full(B, CAP, np.int32)

stream = torch.cuda.Stream()
solver = api.PnPSolver(B, N, 100, stream=stream.cuda_stream)
with torch.cuda.stream(stream):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_ld, d_cd, d_lp, d_cp = up(ld), up(cd), up(lp.view(np.uint8).reshape(B, CAP, 28)), up(cp.view(np.uint8).reshape(B, CAP, 28))
    d_nl, d_nc, d_xy, d_lm, d_pos = up(cnt_rows), up(cnt_rows.copy()), up(xy), up(lm), up(pos)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device="cuda")
    d_ti, d_dist, d_pairs, d_np, d_valid = z(B, CAP), z(B, CAP), z(B, CAP, 2), z(B), z(B, N, 2)
    d_p3, d_p2, d_cnt, d_mst = z(B, N, 3, dt=torch.float32), z(B, N, 2, dt=torch.float32), z(B), z(B)
    pose, flag, ninl, st = z(B, 7, dt=torch.float64), z(B, N, dt=torch.uint8), z(B), z(B)
    h_ti = torch.zeros(B, CAP, dtype=torch.int32).pin_memory(); h_dist = torch.zeros(B, CAP, dtype=torch.int32).pin_memory()
    h_p3 = torch.zeros(B, N, 3, dtype=torch.float32).pin_memory(); h_p2 = torch.zeros(B, N, 2, dtype=torch.float32).pin_memory()
    h_cnt = torch.zeros(B, dtype=torch.int32).pin_memory()
S = stream.cuda_stream


def verify():
    solver.verify_batch(d_p3.data_ptr(), d_p2.data_ptr(), d_cnt.data_ptr(), B, K, pose.data_ptr(), flag.data_ptr(), ninl.data_ptr(), st.data_ptr())


def match_device():
    api.loop_match_batch(d_ld.data_ptr(), d_nl.data_ptr(), d_cd.data_ptr(), d_nc.data_ptr(), d_lp.data_ptr(), d_cp.data_ptr(), B, CAP, d_xy.data_ptr(),
                         d_lm.data_ptr(), N, d_pos.data_ptr(), N, N, 10, N, d_ti.data_ptr(), d_dist.data_ptr(), d_pairs.data_ptr(), d_np.data_ptr(),
                         d_valid.data_ptr(), d_p3.data_ptr(), d_p2.data_ptr(), d_cnt.data_ptr(), d_mst.data_ptr(), S)


def match_host():
    """the previous commit's path up to verify_batch's inputs: two host synchronisations around per-candidate host work"""
    api.hamming_match_batch(d_ld.data_ptr(), d_nl.data_ptr(), d_cd.data_ptr(), d_nc.data_ptr(), B, CAP, d_ti.data_ptr(), d_dist.data_ptr(), S)
    with torch.cuda.stream(stream):
        h_ti.copy_(d_ti, non_blocking=True); h_dist.copy_(d_dist, non_blocking=True)
    stream.synchronize()
    ti, dist, p3, p2, c = h_ti.numpy(), h_dist.numpy(), h_p3.numpy(), h_p2.numpy(), h_cnt.numpy()
    for b in range(B):
        pairs = api.match_feature_pairs(ti[b], dist[b], lp[b], cp[b])
        c[b] = 0
        if len(pairs) >= 10:
            valid = pairs[lm[b][pairs[:, 1]] >= 0]
            c[b] = len(valid)
            p3[b, :c[b]] = pos[b][lm[b][valid[:, 1]]]; p2[b, :c[b]] = xy[b][valid[:, 0]]
    with torch.cuda.stream(stream):
        d_p3.copy_(h_p3, non_blocking=True); d_p2.copy_(h_p2, non_blocking=True); d_cnt.copy_(h_cnt, non_blocking=True)


def new():
    match_device(); verify()


def old():
    match_host(); verify()


def timed(fn):
    t = time.perf_counter()
    for _ in range(REPS):
        fn()
        stream.synchronize()
    return (time.perf_counter() - t) / REPS * 1e3


def snapshot():
    stream.synchronize()
    return [x.cpu().numpy().copy() for x in (d_cnt, pose, flag, ninl, st)]


old(); ref = snapshot()
for x in (d_p3, d_p2, d_cnt, pose, flag, ninl, st):
    x.zero_()
new(); got = snapshot()
same = all(np.array_equal(a, b) for a, b in zip(got, ref))
print(f"results: counts {got[0].tolist()} inliers {got[3].tolist()} status {got[4].tolist()}; device path equals host path bit for bit: {same}", flush=True)
assert same
graph = api.StepGraph.record(S, [], new)
forms = {"loop_match_batch + verify_batch": new, "the same, replayed from a graph": lambda: graph.launch(S), "loop_match_batch only": match_device,
         "previous path + verify_batch": old, "previous path up to the upload only": match_host, "verify_batch only": verify}
for fn in forms.values():                            # warm-up of every form
    timed(fn)
times = {k: [] for k in forms}
for _ in range(ROUNDS):
    for k, fn in forms.items():
        times[k].append(timed(fn))
for k, v in times.items():
    print(f"{k:38s} median {np.median(v):8.3f} ms per {B} candidates   (min {min(v):.3f}, max {max(v):.3f}, {ROUNDS} rounds x {REPS} calls)", flush=True)
print(f"clock {api.shader_clock_mhz(S):.0f} MHz, build {api.build_id()}")
