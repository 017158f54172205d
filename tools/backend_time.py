"""Times Backend::OptimizeActiveMap for 64 active maps of 7 key-frames x 300 map points on the GPU box: one Backend.optimize_batch (device tables, three
launches, nothing read back) against the host path on the same maps, 64 x api.ba_flatten_window + packing + upload + one
api.ba_optimize_active_map_batch + download of poses, points, chi2 and flags.  The host path's container surgery after the solve (chain.py:602-619) is NOT
in its span: it is host work the batch call also replaces, so the comparison favours the host path.

Host clock around calls that end in a device synchronise; the batch form restores its in/out tables by device-to-device copies on its stream before every
call, inside the timed span.  Both forms are warmed up, then timed 20 times each in alternation; medians with min - max go to
profiles/backend_time.json (--out names another file).  The maps come from tests/backend_ref.py's make_map.  There is no pass / fail ratio: the tool reports."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
from __graft_entry__ import load_package  # noqa: E402
import backend_ref as br  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backend_time.json"))
ap.add_argument("--maps", type=int, default=64)
args = ap.parse_args()
pkg = load_package(); api, synth = pkg.api, pkg.synth
B, NKF, NMP, REPS = args.maps, 7, 300, 20

made = [br.make_map(synth, 0x700 + s, n_kf=NKF, n_mp=NMP) for s in range(B)]
maps, K = [m[0] for m in made], made[0][1]
packed = [br.pack(m) for m in maps]
KF_CAP, MP_CAP, OBS_CAP = NKF, max(len(p["mp_id"]) for p in packed), max(len(p["obs_mp"]) for p in packed) + 8
host = br.pack_batch(maps, KF_CAP, MP_CAP, OBS_CAP)
stream = torch.cuda.Stream()
be = api.Backend(B, KF_CAP, MP_CAP, OBS_CAP, stream=stream.cuda_stream)
IN_OUT = ("kf_pose", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")
with torch.cuda.stream(stream):
    d = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    keep = {k: d[k].clone() for k in IN_OUT}
    o = dict(obs_report=torch.zeros(B, OBS_CAP, dtype=torch.uint8, device="cuda"), mp_report=torch.zeros(B, MP_CAP, dtype=torch.uint8, device="cuda"),
             new_outlier=torch.zeros(B, MP_CAP, dtype=torch.int32, device="cuda"), n_new=torch.zeros(B, dtype=torch.int32, device="cuda"),
             obs_chi2=torch.zeros(B, OBS_CAP, dtype=torch.float64, device="cuda"), rounds=torch.zeros(B, dtype=torch.int32, device="cuda"),
             n_out=torch.zeros(B, dtype=torch.int32, device="cuda"), status=torch.zeros(B, dtype=torch.int32, device="cuda"))


def batch():
    with torch.cuda.stream(stream):
        for k, v in keep.items():
            d[k].copy_(v)
    be.optimize_batch(*[d[k].data_ptr() for k in ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv",
                                                   "obs_tag", "n_obs")], B, K,
                      *[o[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2", "rounds", "n_out", "status")])


flat_args = [br.host_flatten_args(m)[0] for m in maps]           # the Map's containers as id arrays: what a host caller holds anyway
scratch = torch.zeros(B * OBS_CAP * 18, dtype=torch.float64, device="cuda")


def host_path():
    poses = np.zeros((B, KF_CAP, 7)); pts = np.zeros((B, MP_CAP, 3)); ep = np.zeros((B, OBS_CAP), np.int32); el = np.zeros((B, OBS_CAP), np.int32)
    obs = np.zeros((B, OBS_CAP, 2)); fixed = np.zeros((B, MP_CAP), np.uint8); sizes = np.zeros((B, 3), np.int32)
    for w, (a, p) in enumerate(zip(flat_args, packed)):
        f = api.ba_flatten_window(*a)
        P, L, E = len(f["pose_src"]), len(f["pt_src"]), len(f["edge_pose"])
        poses[w, :P] = p["kf_pose"][f["pose_src"]]; pts[w, :L] = p["mp_pos"][f["pt_src"]]; ep[w, :E] = f["edge_pose"]; el[w, :E] = f["edge_pt"]
        obs[w, :E] = f["edge_obs"]; fixed[w, :L] = f["fixed"]; sizes[w] = (P, L, E)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(a).cuda() for a in (poses, pts, ep, el, obs, fixed, sizes)]
        chi = torch.empty(B, OBS_CAP, dtype=torch.float64, device="cuda"); out = torch.empty(B, OBS_CAP, dtype=torch.uint8, device="cuda")
        rd = torch.empty(B, dtype=torch.int32, device="cuda"); no = torch.empty(B, dtype=torch.int32, device="cuda"); st = torch.empty(B, dtype=torch.int32, device="cuda")
        api.ba_optimize_active_map_batch(*[x.data_ptr() for x in t], B, KF_CAP, MP_CAP, OBS_CAP, K, 5.991, 5.991, 5, 10, scratch.data_ptr(), chi.data_ptr(),
                                         out.data_ptr(), rd.data_ptr(), no.data_ptr(), st.data_ptr(), stream.cuda_stream)
        return [x.cpu().numpy() for x in (t[0], t[1], chi, out, rd, no, st)], sizes


def timed(fn, sync):
    t = time.perf_counter()
    fn()
    if sync:
        stream.synchronize()
    return (time.perf_counter() - t) * 1e3


batch(); stream.synchronize()
status = o["status"].cpu().numpy(); rounds = o["rounds"].cpu().numpy()
(hp, hx, hchi, hout, hrd, hno, hst), sizes = host_path()
same = all(np.array_equal(d["kf_pose"][b, :NKF].cpu().numpy(), hp[b, :NKF]) for b in range(B)) and np.array_equal(rounds, hrd) and \
    np.array_equal(o["n_out"].cpu().numpy(), hno)
print(f"results: status {sorted(set(status.tolist()))}, rounds {sorted(set(rounds.tolist()))}, edges {int(sizes[:, 2].min())} - {int(sizes[:, 2].max())}, "
      f"landmarks {int(sizes[:, 1].min())} - {int(sizes[:, 1].max())}; poses, rounds and outlier counts of both forms identical: {same}", flush=True)
forms = {"optimize_batch": (batch, True), "host flatten + upload + solve + download": (host_path, False)}
for fn, sync in forms.values():
    for _ in range(3):
        timed(fn, sync)
times = {k: [] for k in forms}
for _ in range(REPS):
    for k, (fn, sync) in forms.items():
        times[k].append(timed(fn, sync))
res = {"workload": f"{B} maps x {NKF} key-frames x {NMP} map points, caps {KF_CAP} / {MP_CAP} / {OBS_CAP}", "status": sorted(set(status.tolist())),
       "edges_min_max": [int(sizes[:, 2].min()), int(sizes[:, 2].max())], "forms_identical": bool(same), "calls_per_form": REPS, "ms": {}}
for k, v in times.items():
    res["ms"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(f"{k:44s} median {np.median(v):9.3f} ms per {B} maps   (min {min(v):.3f}, max {max(v):.3f}, {REPS} calls)", flush=True)
res["clock_mhz"] = float(api.shader_clock_mhz(stream.cuda_stream)); res["build"] = api.build_id()
print(f"clock {res['clock_mhz']:.0f} MHz, build {res['build']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
