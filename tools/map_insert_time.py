"""Times Map::InsertKeyFrame for 64 active maps on the GPU box: one Backend.insert_keyframe_batch (device tables, one launch, nothing read back) at the
sizes of the chain's 44-frame run: 7 -> 8 key-frames with a window of 7 (so one leaves), 450 map points, 7 000 observation rows, 400 features of which 10
name new ids.  The call is timed eager and replayed from a step graph; the yardstick is a device-to-device copy of the same table bytes, the floor for a
call that rewrites its tables.

Every form first restores the in/out tables by device-to-device copies on the stream (a second insert of the same key-frame would be refused), so
"restore" is timed on its own and subtracted.  Host clock around spans that end in a stream synchronise; forms warmed up, then timed 20 times each in
alternation; medians with min - max go to profiles/map_insert_time.json (--out names another file).  There is no pass / fail ratio: the tool reports."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_insert_time.json"))
ap.add_argument("--maps", type=int, default=64)
args = ap.parse_args()
pkg = load_package(); api = pkg.api
B, NKF, NMP, NOBS, NFEAT, NNEW, WINDOW, REPS = args.maps, 7, 450, 7000, 400, 10, 7, 20
KF_CAP, MP_CAP, OBS_CAP, FEAT_CAP = NKF + 1, NMP + 32, NOBS + 512, NFEAT + 16
ACTIVE = api.BACKEND_OBS_ACTIVE


def tables(seed):
    """one map's tables, valid and of the run's sizes: ids ascending with gaps, rows grouped by map point, a third of the rows of key-frames that left"""
    rng = np.random.default_rng([seed, 0x1A5E])
    t = dict(kf_id=np.full(KF_CAP, -1, np.int64), kf_pose=np.zeros((KF_CAP, 7)), mp_id=np.full(MP_CAP, -1, np.int64), mp_pos=np.zeros((MP_CAP, 3)),
             mp_outlier=np.zeros(MP_CAP, np.uint8), obs_mp=np.zeros(OBS_CAP, np.int32), obs_kf=np.full(OBS_CAP, -1, np.int32),
             obs_flags=np.zeros(OBS_CAP, np.uint8), obs_uv=np.zeros((OBS_CAP, 2), np.float32), obs_tag=np.zeros(OBS_CAP, np.int32))
    t["kf_id"][:NKF] = 10 + np.cumsum(rng.integers(1, 3, NKF))
    t["kf_pose"][:, 3] = 1.0
    t["kf_pose"][:NKF, 4:] = rng.uniform(-1, 1, (NKF, 3)) + np.arange(NKF)[:, None] * 0.3
    t["mp_id"][:NMP] = 1000 + np.cumsum(rng.integers(1, 4, NMP))
    t["mp_pos"][:NMP] = rng.uniform(-5, 5, (NMP, 3)) + (0, 0, 15)
    t["obs_mp"][:NOBS] = np.sort(np.concatenate([np.arange(NMP), rng.integers(0, NMP, NOBS - NMP)])).astype(np.int32)
    kf = rng.integers(0, NKF, NOBS).astype(np.int32)
    kf[rng.random(NOBS) < 0.33] = -1
    t["obs_kf"][:NOBS] = kf
    t["obs_flags"][:NOBS] = np.where(kf >= 0, ACTIVE, 0)
    t["obs_uv"][:NOBS] = rng.uniform(0, 1200, (NOBS, 2)); t["obs_tag"][:NOBS] = np.arange(NOBS)
    feat_id = np.full(FEAT_CAP, -1, np.int64)
    feat_id[:NFEAT - NNEW] = rng.permutation(t["mp_id"][:NMP])[:NFEAT - NNEW]
    feat_id[NFEAT - NNEW:NFEAT] = t["mp_id"][NMP - 1] + 1 + np.arange(NNEW)
    feat_id[:NFEAT] = rng.permutation(feat_id[:NFEAT])
    new_pose = np.array([0, 0, 0, 1.0, *(rng.uniform(-1, 1, 3) + NKF * 0.3)])
    ins = dict(new_kf_id=np.int64(t["kf_id"][NKF - 1] + 1), new_kf_pose=new_pose, feat_mp_id=feat_id, feat_mp_pos=rng.uniform(-5, 5, (FEAT_CAP, 3)) + (0, 0, 15),
               feat_uv=rng.uniform(0, 1200, (FEAT_CAP, 2)).astype(np.float32), feat_tag=(10 ** 6 + np.arange(FEAT_CAP)).astype(np.int32),
               feat_flags=np.zeros(FEAT_CAP, np.uint8))
    return t, ins


made = [tables(s) for s in range(B)]
host = {k: np.stack([m[0][k] for m in made]) for k in made[0][0]}
host.update(n_kf=np.full(B, NKF, np.int32), n_mp=np.full(B, NMP, np.int32), n_obs=np.full(B, NOBS, np.int32))
inp = {k: np.stack([m[1][k] for m in made]) for k in made[0][1]}
inp["n_feat"] = np.full(B, NFEAT, np.int32)
stream = torch.cuda.Stream()
be = api.Backend(B, KF_CAP, MP_CAP, OBS_CAP, stream=stream.cuda_stream)
TABLE_ARGS = ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")
with torch.cuda.stream(stream):
    d = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    keep = {k: v.clone() for k, v in d.items()}
    spare = {k: torch.empty_like(v) for k, v in d.items()}
    di = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    o = dict(feat_row=torch.zeros(B, FEAT_CAP, dtype=torch.int32, device="cuda"), mp_new_row=torch.zeros(B, MP_CAP, dtype=torch.int32, device="cuda"),
             removed_kf_id=torch.zeros(B, dtype=torch.int64, device="cuda"), removed_kf_row=torch.zeros(B, dtype=torch.int32, device="cuda"),
             dis=torch.zeros(B, KF_CAP, dtype=torch.float64, device="cuda"), status=torch.ones(B, dtype=torch.int32, device="cuda"))
table_bytes = int(sum(v.numel() * v.element_size() for v in d.values()))


def restore():
    with torch.cuda.stream(stream):
        for k, v in keep.items():
            d[k].copy_(v)


def insert():
    be.insert_keyframe_batch(*[d[k].data_ptr() for k in TABLE_ARGS],
                             *[di[k].data_ptr() for k in ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags", "n_feat")],
                             FEAT_CAP, None, None, None, None, None, None, 0, None, None, 0, B, WINDOW, 0.2,
                             *[o[k].data_ptr() for k in ("feat_row", "mp_new_row", "removed_kf_id", "removed_kf_row", "dis", "status")])


def copy():
    with torch.cuda.stream(stream):
        for k, v in d.items():
            spare[k].copy_(v)


restore(); insert(); stream.synchronize()
status = o["status"].cpu().numpy()
n_mp, n_obs = d["n_mp"].cpu().numpy(), d["n_obs"].cpu().numpy()
print(f"results: status {sorted(set(status.tolist()))}, key-frames {sorted(set(d['n_kf'].cpu().numpy().tolist()))}, map points {n_mp.min()} - {n_mp.max()}, "
      f"rows {n_obs.min()} - {n_obs.max()}", flush=True)
restore(); stream.synchronize()
graph = api.StepGraph.record(stream.cuda_stream, [], insert)
forms = {"restore": lambda: restore(), "restore + copy of the tables": lambda: (restore(), copy()), "restore + insert_keyframe_batch": lambda: (restore(), insert()),
         "restore + insert_keyframe_batch from a step graph": lambda: (restore(), graph.launch(stream.cuda_stream))}


def timed(fn):
    t = time.perf_counter()
    fn()
    stream.synchronize()
    return (time.perf_counter() - t) * 1e3


for fn in forms.values():
    for _ in range(3):
        timed(fn)
times = {k: [] for k in forms}
for _ in range(REPS):
    for k, fn in forms.items():
        times[k].append(timed(fn))
assert (o["status"].cpu().numpy() == 0).all()
res = {"workload": f"{B} maps x {NKF} -> {NKF + 1} key-frames (window {WINDOW}), {NMP} map points, {NOBS} rows, {NFEAT} features ({NNEW} new ids), caps "
                   f"{KF_CAP} / {MP_CAP} / {OBS_CAP}", "status": sorted(set(status.tolist())), "table_bytes": table_bytes, "calls_per_form": REPS, "ms": {}}
for k, v in times.items():
    res["ms"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(f"{k:52s} median {np.median(v):9.3f} ms per {B} maps   (min {min(v):.3f}, max {max(v):.3f}, {REPS} calls)", flush=True)
med = {k: v["median"] for k, v in res["ms"].items()}
res["insert_minus_restore_ms"] = med["restore + insert_keyframe_batch"] - med["restore"]
res["graph_minus_restore_ms"] = med["restore + insert_keyframe_batch from a step graph"] - med["restore"]
res["copy_minus_restore_ms"] = med["restore + copy of the tables"] - med["restore"]
res["insert_over_copy"] = res["insert_minus_restore_ms"] / res["copy_minus_restore_ms"]
print(f"insert {res['insert_minus_restore_ms']:.3f} ms, from a graph {res['graph_minus_restore_ms']:.3f} ms, copy {res['copy_minus_restore_ms']:.3f} ms: "
      f"{res['insert_over_copy']:.2f} x the copy of {table_bytes / 1e6:.1f} MB")
res["clock_mhz"] = float(api.shader_clock_mhz(stream.cuda_stream)); res["build"] = api.build_id()
print(f"clock {res['clock_mhz']:.0f} MHz, build {res['build']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
