"""Times the device map archive against the host round trip it replaces, for 16 and 64 streams at the reference's window: 7 key-frames, 600 active map
points (4 observation rows each), an archive of 500 key-frames and 30 000 map points per stream.

Device form, one launch each, nothing read back: MapArchive.update_batch after an insert, update_batch after an optimise, loop_inputs_batch.  One such
call is shorter than the host's cost of enqueuing it, so each is timed as a burst of 50 calls in one span and reported per call (after the first call of
a burst every row is found, nothing is appended).  The appending update (1 new key-frame with its edge, 10 new points) is timed one call per span behind
device-to-device copies that put the three archive counts back; that restore is timed on its own.
Host form: download the thirteen back-end tables, run tests/map_archive_ref.py's bookkeeping (update after an optimise + loop_inputs, plain Python,
per stream), upload myslam_loop_correct_batch's inputs (poses, edges, points, the index arrays).

Host clock around spans that end in a synchronise; forms warmed up, then timed 25 times each in alternation; medians with min - max go to
profiles/map_archive_time.json (--out names another file).  There is no pass / fail ratio: the tool reports.  Not measured: the per-kernel split inside
a call, and archives near point_cap."""
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
import map_archive_ref as mr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_archive_time.json"))
ap.add_argument("--streams", type=int, nargs="+", default=[16, 64])
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api = pkg.api; chain = pkg.chain
NKF, NMP, ROWS, AKF, AMP, NEWMP = 7, 600, 4, 500, 30000, 10
BE_CAPS = (8, 640, 2816)
CAPS = (512, 520, 32768)
ACTIVE_CAP = 10
BURST = 50


def one_map():
    """-> (the arguments of MapArchive.load, the back end's tables after the insert of key-frame AKF, unpadded)"""
    rng = np.random.default_rng(0xA7C1)
    kf_id = 10 + 2 * np.arange(AKF + 1, dtype=np.int64)
    pose = np.zeros((AKF + 1, 7)); pose[:, 3] = 1.0; pose[:, 4:] = np.cumsum(rng.uniform(0.05, 0.3, (AKF + 1, 3)), 0)
    meas = np.array([mr.edge_meas(chain, pose[i], pose[i - 1]) for i in range(1, AKF)])
    mp_id = 1000 + 3 * np.arange(AMP + NEWMP, dtype=np.int64)
    pos = rng.uniform(-50, 50, (AMP + NEWMP, 3))
    load = dict(kf_id=kf_id[:AKF], kf_pose=pose[:AKF], edge_v0=np.arange(1, AKF, dtype=np.int32), edge_v1=np.arange(0, AKF - 1, dtype=np.int32), meas=meas,
                mp_id=mp_id[:AMP], mp_pos=pos[:AMP], mp_first_kf=rng.integers(0, AKF, AMP).astype(np.int32), mp_state=(rng.random(AMP) < 0.1).astype(np.uint8) * 2)
    rows = np.sort(np.r_[rng.choice(np.arange(AMP - 3000, AMP), NMP - NEWMP, replace=False), np.arange(AMP, AMP + NEWMP)])
    obs_mp = np.repeat(np.arange(NMP, dtype=np.int32), ROWS)
    obs_kf = np.sort(rng.integers(0, NKF, (NMP, ROWS)), 1).astype(np.int32)
    obs_kf[rng.random(NMP) < 0.33, 0] = -1
    obs_kf = obs_kf.reshape(-1)
    be = dict(kf_id=kf_id[AKF - NKF + 1:AKF + 1], kf_pose=pose[AKF - NKF + 1:AKF + 1], mp_id=mp_id[rows], mp_pos=pos[rows] + 0.125, obs_mp=obs_mp, obs_kf=obs_kf,
              obs_flags=np.where(obs_kf >= 0, api.BACKEND_OBS_ACTIVE, 0).astype(np.uint8))
    return load, be


class DevArray:
    """a device pointer of the archive's view as something torch can wrap (the CUDA array interface)"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr=typestr, data=(int(ptr), False), version=2)


def measure(B):
    load, be = one_map()
    stream = torch.cuda.Stream()
    arc = api.MapArchive(B, *CAPS, BE_CAPS[1], stream=stream.cuda_stream)
    for b in range(B):
        arc.load(b, **load)
    kc, mc, oc = BE_CAPS
    T = dict(kf_id=np.zeros((B, kc), np.int64), kf_pose=np.zeros((B, kc, 7)), n_kf=np.full(B, NKF, np.int32), mp_id=np.zeros((B, mc), np.int64),
             mp_pos=np.zeros((B, mc, 3)), mp_outlier=np.zeros((B, mc), np.uint8), n_mp=np.full(B, NMP, np.int32), obs_mp=np.zeros((B, oc), np.int32),
             obs_kf=np.zeros((B, oc), np.int32), obs_flags=np.zeros((B, oc), np.uint8), obs_uv=np.zeros((B, oc, 2), np.float32),
             obs_tag=np.zeros((B, oc), np.int32), n_obs=np.full(B, NMP * ROWS, np.int32))
    for k, v in be.items():
        T[k][:, :len(v)] = v
    d = {k: torch.from_numpy(v).cuda() for k, v in T.items()}
    zero = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.zeros(B, dtype=torch.int32, device="cuda")
    report = torch.zeros((B, mc), dtype=torch.uint8, device="cuda")
    cur = torch.full((B,), int(be["kf_id"][-1]), dtype=torch.int64, device="cuda"); loop = torch.full((B,), int(load["kf_id"][40]), dtype=torch.int64, device="cuda")
    lo = dict(active=torch.zeros((B, ACTIVE_CAP), dtype=torch.int32, device="cuda"), n_active=zero.clone(), cur=zero.clone(), loop=zero.clone(),
              first_active=torch.zeros((B, CAPS[2]), dtype=torch.int32, device="cuda"), first_kf=torch.zeros((B, CAPS[2]), dtype=torch.int32, device="cuda"),
              n_points=zero.clone())
    p = lambda t: t.data_ptr()
    v = arc.view()
    try:
        counts = [torch.as_tensor(DevArray(ptr, B, "<i4"), device="cuda") for ptr in (v.n_kf, v.n_edges, v.n_mp)]
    except Exception as e:                                                  # no way to wrap the pointers: every update after the first finds all rows
        print("counts are not restored:", repr(e))
        counts = []
    saved = [torch.full((B,), n, dtype=torch.int32, device="cuda") for n in (AKF, AKF - 1, AMP)]

    def restore():
        for c, s in zip(counts, saved):
            c.copy_(s)

    def update(mode):
        arc.update_batch(mode, p(d["kf_id"]), p(d["kf_pose"]), p(d["n_kf"]), kc, p(d["mp_id"]), p(d["mp_pos"]), p(d["n_mp"]), mc, p(d["obs_mp"]), p(d["obs_kf"]),
                         p(d["obs_flags"]), p(d["n_obs"]), oc, p(zero), None, None, 0, p(report), B, p(st))

    def inputs():
        arc.loop_inputs_batch(p(d["kf_id"]), p(d["n_kf"]), kc, p(d["mp_id"]), p(d["n_mp"]), mc, p(d["obs_mp"]), p(d["obs_kf"]), p(d["obs_flags"]), p(d["n_obs"]), oc,
                              p(cur), p(loop), p(zero), ACTIVE_CAP, B, *[p(lo[k]) for k in ("active", "n_active", "cur", "loop", "first_active", "first_kf", "n_points")])

    # the host's own map: the walk's archive after the insert, one per stream
    walks = []
    for b in range(B):
        a = mr.Archive()
        a.kf_id = [int(x) for x in load["kf_id"]]; a.kf_pose = [x for x in load["kf_pose"]]
        a.edge_v0 = list(load["edge_v0"]); a.edge_v1 = list(load["edge_v1"]); a.meas = [x for x in load["meas"]]
        a.mp_id = [int(x) for x in load["mp_id"]]; a.mp_pos = [x for x in load["mp_pos"]]; a.mp_first_kf = list(load["mp_first_kf"]); a.mp_state = list(load["mp_state"])
        a.mp_gone_kf = [-1] * AMP; a.mp_win_mask = [0] * AMP
        assert mr.update(chain, a, mr.AFTER_INSERT, be, 0) == mr.UPDATED
        walks.append(a)

    def host_form():
        h = {k: t.cpu().numpy() for k, t in d.items()}                      # the thirteen tables
        up = []
        for b, a in enumerate(walks):
            t = {k: h[k][b, :len(be[k])] for k in be}
            mr.update(chain, a, mr.AFTER_OPTIMIZE, t, 0, mp_report=np.zeros(NMP, np.uint8))
            up.append((a.arrays(), mr.loop_inputs(a, t, int(be["kf_id"][-1]), int(load["kf_id"][40]), 0)))
        for name in ("kf_pose", "edge_v0", "edge_v1", "meas", "mp_pos"):
            torch.from_numpy(np.stack([x[0][name] for x in up])).cuda()
        for name in ("active", "first_active", "first_kf"):
            torch.from_numpy(np.stack([x[1][name] for x in up])).cuda()
        torch.from_numpy(np.array([[x[1]["cur"], x[1]["loop"], x[1]["n_points"]] for x in up], np.int32)).cuda()

    def burst(body, restored=False):
        def f():
            with torch.cuda.stream(stream):
                if restored:
                    restore()
                for _ in range(1 if restored else BURST):
                    body()
        return f

    # a single call is shorter than the host's cost of enqueuing it: the device forms are timed as bursts of BURST calls in one span, reported per call.
    # In a burst every row is found (nothing is appended after the first call); the appending call is timed once per span behind its restore.
    forms = {"update after insert, per call of a burst": burst(lambda: update(mr.AFTER_INSERT)),
             "update after optimise, per call of a burst": burst(lambda: update(mr.AFTER_OPTIMIZE)),
             "loop_inputs, per call of a burst": burst(inputs),
             "restore of the counts, one span": burst(lambda: None, True),
             "restore + appending update after insert, one span": burst(lambda: update(mr.AFTER_INSERT), True),
             "host: download 13 tables + walk + upload": host_form}
    ms = {k: [] for k in forms}
    stream.wait_stream(torch.cuda.current_stream())
    for k, f in forms.items():                                              # warm-up
        f(); torch.cuda.synchronize()
    status = st.cpu().numpy().tolist()
    for _ in range(args.reps):
        for k, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / (BURST if "burst" in k else 1))
    out = {k: dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x))) for k, x in ms.items()}
    med = lambda k: out[k]["median"]
    derived = dict(update_after_insert_ms=med("update after insert, per call of a burst"), update_after_optimise_ms=med("update after optimise, per call of a burst"),
                   loop_inputs_ms=med("loop_inputs, per call of a burst"), host_ms=med("host: download 13 tables + walk + upload"))
    derived["device_three_calls_ms"] = derived["update_after_insert_ms"] + derived["update_after_optimise_ms"] + derived["loop_inputs_ms"]
    got = arc.get(B - 1)
    assert len(got["kf_id"]) == AKF + 1 and len(got["mp_id"]) == AMP + NEWMP and len(got["edge_v0"]) == AKF, "the timed update did not append"
    return dict(streams=B, status=sorted(set(status)), appends_every_time=bool(counts), ms=out, derived=derived)


res = dict(workload=f"{NKF} key-frames, {NMP} active map points x {ROWS} rows, archive of {AKF} key-frames and {AMP} map points per stream; caps {BE_CAPS} / {CAPS}",
           calls_per_form=args.reps, runs=[measure(B) for B in args.streams], clock_mhz=api.shader_clock_mhz(), build=api.build_id())
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({r["streams"]: r["derived"] for r in res["runs"]}, indent=1))
