"""Times one key-frame of the device chain at a batch of 64 maps (--batch) without and with the observation archive's three launches, by the method of
tools/link_upkeep_time.py: host clock around spans that end in a synchronise, warmed up, the two forms in alternation, medians with min - max.
    parent   insert_keyframe_batch -> MapArchive.update_batch -> optimize_batch -> MapArchive.update_batch
    new      ObsArchive.prior_rows_batch -> the same insert -> map update -> ObsArchive.update_batch -> optimise -> map update -> ObsArchive.update_batch
Every map is backend_ref.make_map's (6 key-frames at a window of 6, 60 map points, so the 7th key-frame makes one leave and points with it), with 40
stored map points of 2 rows each outside the table, 3 of which the new key-frame names.  Before every span the tables, the map archive and the
observation archive of every item are put back (outside the span), so every span does the same work; the parent form's insert reads the prior arrays
a prior_rows call left there before the timing began.  Results go to profiles/obs_archive_time.json (--out names another file).  The tool reports;
there is no pass / fail ratio."""
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
import map_archive_ref as mr  # noqa: E402
import obs_archive_ref as oa  # noqa: E402
from test_gpu_map_archive import Dev  # noqa: E402
from test_gpu_map_histories import LOAD, OPT_OUT  # noqa: E402
from test_gpu_map_insert import TABLE_ARGS, Run, next_keyframe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_archive_time.json"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api = pkg.api
chain, synth = pkg.chain, pkg.synth
B, WINDOW, N_STORED, ROW_CAP = args.batch, 6, 40, 512
BE_CAPS, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP, ARCH_CAPS = (8, 160, 1600), 64, 32, 6, (16, 15, 256)
PRIOR = ("prior_mp_id", "prior_kf_id", "prior_uv", "prior_tag", "prior_flags")
rng = np.random.default_rng(0x0A7C)

maps, inss, archives, stores = [], [], [], []
for b in range(B):
    m, K, _ = br.make_map(synth, 0x400 + b, n_kf=6, n_mp=60)
    stored = [(1 + j, [(3, np.float32(10 + j), np.float32(20.5), 5000 + 2 * j, 0), (7, np.float32(11 + j), np.float32(21.5), 5001 + 2 * j, br.OUTLIER * (j % 5 == 0))])
              for j in range(N_STORED)]
    a, w0 = mr.Archive(), br.Map()                                          # the map archive: the stored points were active under key-frames 3 and 7
    for k in (3, 7, 11):
        w0.kfs[k] = np.array([0, 0, 0, 1, 0.1 * k, 0, 0], float)
    for mid, rows in stored:
        mp = br.MapPoint(mid, (0.1 * mid, 0.2, 12.0))
        mp.obs = [br.Obs(r[0], r[1], r[2], bool(r[4]), r[3]) for r in rows]; mp.active_obs = list(mp.obs)
        w0.mps[mid] = mp
    assert mr.update(chain, a, mr.AFTER_INSERT, br.pack(w0), 0, caps=ARCH_CAPS) == mr.UPDATED
    assert mr.update(chain, a, mr.AFTER_INSERT, br.pack(m), 0, caps=ARCH_CAPS) == mr.UPDATED
    ins = next_keyframe(chain, m, K, 0, rng)
    ins.feats = [f for f in ins.feats if f[0] < 0 or f[0] in m.mps or f[0] > a.mp_id[-1]]     # ids come from a counter
    ins.feats += [(mid, (0.1 * mid, 0.2, 12.0), (np.float32(300 + mid), np.float32(100.0)), 7000 + mid, False) for mid in (2, 17, 33)]
    ins.priors = []
    kf_of = lambda o: o.kf
    rows_of = lambda mp: [(kf_of(o), o.u, o.v, o.tag, br.OUTLIER if o.outlier else 0) for o in mp.obs]
    maps.append(m); inss.append(ins); archives.append(a)
    stores.append(oa.Store.loaded(ROW_CAP, stored, sorted(m.mps), [rows_of(m.mps[i]) for i in sorted(m.mps)]))

r = Run(api, maps, inss, WINDOW, 0.2, caps=(BE_CAPS, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP))
dev = Dev(api, B, ARCH_CAPS, BE_CAPS, r.stream)
dev.h.attach_solve(*r.h.solve_view())
obs = api.ObsArchive(dev.h, B, BE_CAPS[2], ROW_CAP, stream=r.stream.cuda_stream)
full = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
oo = dict(obs_report=full((B, BE_CAPS[2]), torch.uint8), mp_report=full((B, BE_CAPS[1]), torch.uint8), new_outlier=full((B, BE_CAPS[1]), torch.int32),
          n_new=full((B,), torch.int32), obs_chi2=full((B, BE_CAPS[2]), torch.float64), rounds=full((B,), torch.int32), n_out=full((B,), torch.int32),
          status=full((B,), torch.int32))
ostatus, pstatus = full((B,), torch.int32), full((B,), torch.int32)
p = lambda t: t.data_ptr()
d, di = r.d, r.di
arch_args = [[a.arrays()[k] for k in LOAD] for a in archives]
obs_args = [st.load_args(a) for st, a in zip(stores, archives)]


def put_back():
    r.restore()
    r.stream.synchronize()
    for b in range(B):
        dev.h.load(b, *arch_args[b])
        obs.load(b, *obs_args[b])


def prior_rows():
    obs.prior_rows_batch(p(di["feat_mp_id"]), p(di["n_feat"]), FEAT_CAP, p(d["mp_id"]), p(d["n_mp"]), BE_CAPS[1], B, *[p(di[k]) for k in PRIOR], p(di["n_prior"]),
                         PRIOR_CAP, p(pstatus))


def obs_update(mode, be_status, report):
    obs.update_batch(mode, *[p(d[k]) for k in TABLE_ARGS], *BE_CAPS, p(be_status), p(dev.status), report, B, p(ostatus))


def key_frame(new):
    if new:
        prior_rows()
    r.enqueue()
    dev.update(mr.AFTER_INSERT, d, r.o["status"], di["outlier_mp_id"], di["n_outlier"], OUTLIER_CAP)
    if new:
        obs_update(mr.AFTER_INSERT, r.o["status"], None)
    r.h.optimize_batch(*[p(d[k]) for k in TABLE_ARGS], B, K, *[p(oo[k]) for k in OPT_OUT])
    dev.update(mr.AFTER_OPTIMIZE, d, oo["status"], report=oo["mp_report"])
    if new:
        obs_update(mr.AFTER_OPTIMIZE, oo["status"], p(oo["obs_report"]))


r.stream.wait_stream(torch.cuda.current_stream())
put_back()
key_frame(True)                                                             # warm-up, and what the work is
torch.cuda.synchronize()
counts = dict(insert_ok=int((r.o["status"] == 0).sum()), optimise_done=int((oo["status"] == 0).sum()), obs_updated=int((ostatus == 0).sum()),
              prior_rows=int(di["n_prior"].sum()), prior_ok=int((pstatus == 0).sum()),
              stored_points_after=int(sum(len(obs.get(b)["seg_mp_id"]) for b in range(B))), reclaims=int(sum(obs.get(b)["n_reclaims"] for b in range(B))))
assert counts["insert_ok"] == counts["optimise_done"] == counts["obs_updated"] == counts["prior_ok"] == B and counts["prior_rows"] == 6 * B, counts
prior_inp = {k: di[k].clone() for k in PRIOR + ("n_prior",)}               # restore() puts the host's empty priors back: the parent form gets these
forms = {"parent: insert + update + optimise + update": False, "new: + prior_rows + 2 obs updates": True}
ms = {k: [] for k in forms}
for rep in range(args.reps + 2):
    for k, new in forms.items():
        put_back()
        with torch.cuda.stream(r.stream):
            for name, v in prior_inp.items():
                di[name].copy_(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        key_frame(new)
        torch.cuda.synchronize()
        if rep >= 2:
            ms[k].append((time.perf_counter() - t0) * 1e3)
res = {"workload": f"batch {B}: maps of 6 key-frames and 60 map points at a window of {WINDOW}, a 7th key-frame of ~55 features, {N_STORED} stored points of 2 rows, "
                   f"3 of them named; caps {BE_CAPS}, row_cap {ROW_CAP}", "spans": args.reps, "counts": counts,
       "ms_per_key_frame": {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()}}
a, b_ = [res["ms_per_key_frame"][k] for k in forms]
res["added_us_median"] = (b_["median"] - a["median"]) * 1e3
res["new_median_within_parent_band"] = bool(a["min"] <= b_["median"] <= a["max"])
for k, v in res["ms_per_key_frame"].items():
    print(f"{k:46s} median {v['median'] * 1e3:9.1f} us   (min {v['min'] * 1e3:.1f}, max {v['max'] * 1e3:.1f}; {args.reps} spans)", flush=True)
print(f"added by the three launches: {res['added_us_median']:.1f} us (medians); inside the parent's band: {res['new_median_within_parent_band']}")
res["clock_mhz"] = float(api.shader_clock_mhz(r.stream.cuda_stream)); res["build"] = api.build_id()
print(f"counts {counts}, clock {res['clock_mhz']:.0f} MHz, build {res['build']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
