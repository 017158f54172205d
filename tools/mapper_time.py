"""Times one key-frame of a bank at 64 and at 256 maps through three forms, by the method of tools/obs_archive_time.py (host clock around spans that end in
a synchronise, warmed up, the forms in alternation on one box in one session, medians with min - max):
    (a) separate   the eleven launches through the entry points the mapper composes: ObsArchive.prior_rows_batch -> Backend.insert_keyframe_batch ->
                   MapArchive.update_batch -> ObsArchive.update_batch -> Backend.optimize_batch (3) -> MapArchive.update_batch -> ObsArchive.update_batch ->
                   Tracker.clear_links_batch -> Tracker.update_from_map, every item taking the key-frame
    (b) mapper     Mapper.keyframe_batch on the same items (those launches between the gate and the status launch: 13)
    (c) one in six Mapper.keyframe_batch with five items in six idle (MYSLAM_TRACKER_NO_TURN)
Every form has its own state and every span is a NEW key-frame of a steady rolling history, so nothing is put back: key-frame j (a pure translation, 0.25 m a
key-frame — above min_dis_th, so the oldest key-frame leaves —, window 3) sees 96 map points, ids 32 j .. 32 j + 95, each therefore seen by three consecutive key-frames before it leaves the table alive and is
stored; pixels are the projections with a deterministic +-0.3 px.  All items of a bank get the same key-frame (an item's work does not depend on its
neighbours).  The tracker's streams are as created (not running), so its two launches find nothing to do in (a) and in (b) alike.
Results go to profiles/mapper_time.json (--out names another file).  The tool reports; there is no pass / fail ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapper_time.json"))
ap.add_argument("--banks", type=int, nargs="+", default=[64, 256])
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api = pkg.api
K = (718.856, 718.856, 607.1928, 185.2157)
WINDOW, NF, STEP, WARM = 3, 96, 32, 5
BE_CAPS, FEAT_CAP, PRIOR_CAP = (4, 256, 1024), 128, 64
TABLES = api.BE_TABLES
TURN_DT = dict(new_kf_id=torch.int64, new_kf_pose=torch.float64, feat_mp_id=torch.int64, feat_mp_pos=torch.float64, feat_uv=torch.float32, feat_tag=torch.int32,
               feat_flags=torch.uint8, n_feat=torch.int32, outlier_mp_id=torch.int64, n_outlier_mp=torch.int32, report=torch.int32)


def keyframe(j):
    """key-frame j of the rolling history as one item's rows of a turn's output set"""
    ids = np.arange(STEP * j, STEP * j + NF, dtype=np.int64)
    pos = np.stack([0.25 * (ids // STEP) + ((ids * 37) % 96) / 16.0 - 3.0, ((ids * 11) % 50) / 25.0 - 1.0, 8.0 + (ids % 5)], 1).astype(np.float64)
    tx = -0.25 * j                                                           # Tcw of a camera at x = 0.25 j
    pc = pos + np.array([tx, 0.0, 0.0])
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)
    uv += (((ids * 7 + 3 * j) % 13) / 20.0 - 0.3)[:, None] * np.array([1.0, -1.0])
    pad = lambda a, shape, dt: np.concatenate([a, np.zeros((FEAT_CAP - NF,) + shape, dt)]).astype(dt)
    return dict(new_kf_id=np.int64(j), new_kf_pose=np.array([0, 0, 0, 1, tx, 0, 0], np.float64), feat_mp_id=pad(ids, (), np.int64), feat_mp_pos=pad(pos, (3,), np.float64),
                feat_uv=pad(uv.astype(np.float32), (2,), np.float32), feat_tag=pad(np.arange(NF, dtype=np.int32), (), np.int32),
                feat_flags=np.zeros(FEAT_CAP, np.uint8), n_feat=np.int32(NF), outlier_mp_id=np.zeros(2 * FEAT_CAP, np.int64), n_outlier_mp=np.int32(0),
                report=np.zeros(8, np.int32))


class Form:
    """one form's state for a bank of B: turn buffers, its handles, the number of key-frames it has taken"""

    def __init__(self, B, stream, trk, kind, n_calls):
        self.B, self.kind, self.trk, self.j = B, kind, trk, 0
        st = stream.cuda_stream
        arch = (n_calls + 4, n_calls + 4, STEP * (n_calls + 4) + NF)
        row_cap = 3 * arch[2]
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        k0 = keyframe(0)
        self.turn = {k: z((B,) + np.shape(k0[k]), dt) for k, dt in TURN_DT.items()}
        self.status = z((B, api.MAPPER_STATUS_WORDS), torch.int32)
        self.take = torch.ones(B, dtype=torch.bool, device="cuda")
        if kind == "one in six":
            self.take[:] = torch.arange(B, device="cuda") % 6 == 0
        if kind == "separate":
            Kc, M, N = BE_CAPS
            self.be = api.Backend(B, Kc, M, N, stream=st)
            self.map = api.MapArchive(B, *arch, M, stream=st)
            self.obs = api.ObsArchive(self.map, B, N, row_cap, stream=st)
            self.map.attach_solve(*self.be.solve_view())
            shapes = dict(kf_id=((Kc,), torch.int64), kf_pose=((Kc, 7), torch.float64), n_kf=((), torch.int32), mp_id=((M,), torch.int64), mp_pos=((M, 3), torch.float64),
                          mp_outlier=((M,), torch.uint8), n_mp=((), torch.int32), obs_mp=((N,), torch.int32), obs_kf=((N,), torch.int32), obs_flags=((N,), torch.uint8),
                          obs_uv=((N, 2), torch.float32), obs_tag=((N,), torch.int32), n_obs=((), torch.int32))
            self.d = {k: z((B,) + s, dt) for k, (s, dt) in shapes.items()}
            P, F = PRIOR_CAP, FEAT_CAP
            self.prior = [z((B, P), torch.int64), z((B, P), torch.int64), z((B, P, 2), torch.float32), z((B, P), torch.int32), z((B, P), torch.uint8), z(B, torch.int32)]
            self.ins_out = [z((B, F), torch.int32), z((B, M), torch.int32), z(B, torch.int64), z(B, torch.int32), z((B, Kc), torch.float64)]
            self.opt_out = [z((B, N), torch.uint8), z((B, M), torch.uint8), z((B, M), torch.int32), z(B, torch.int32), z((B, N), torch.float64), z(B, torch.int32),
                            z(B, torch.int32)]
            self.st = [z(B, torch.int32) for _ in range(7)]
            self.n_cleared = z(B, torch.int32)
            self.culled = self.be.culled_view()
        else:
            self.m = api.Mapper(B, *BE_CAPS, FEAT_CAP, *arch, row_cap, PRIOR_CAP, stream=st)

    def fill(self):
        """the next key-frame into every item's buffers (outside the span)"""
        kf = keyframe(self.j)
        for k, v in kf.items():
            self.turn[k].copy_(torch.from_numpy(np.ascontiguousarray(v)).cuda().unsqueeze(0).expand_as(self.turn[k]) if np.ndim(v) else torch.full_like(self.turn[k], v.item()))
        if self.kind == "one in six":
            self.turn["report"][:, 0] = torch.where(self.take, 0, api.Tracker.NO_TURN).to(torch.int32)
        self.j += 1

    def call(self):
        t = {k: v.data_ptr() for k, v in self.turn.items()}
        if self.kind != "separate":
            self.m.keyframe_batch(self.trk, t, WINDOW, K, self.status.data_ptr())
            return
        B, (Kc, M, N) = self.B, BE_CAPS
        d = {k: v.data_ptr() for k, v in self.d.items()}
        tabs = [d[k] for k in TABLES]
        s = [x.data_ptr() for x in self.st]
        pr = [x.data_ptr() for x in self.prior]
        self.obs.prior_rows_batch(t["feat_mp_id"], t["n_feat"], FEAT_CAP, d["mp_id"], d["n_mp"], M, B, *pr, PRIOR_CAP, s[0])
        self.be.insert_keyframe_batch(*tabs, t["new_kf_id"], t["new_kf_pose"], t["feat_mp_id"], t["feat_mp_pos"], t["feat_uv"], t["feat_tag"], t["feat_flags"], t["n_feat"],
                                      FEAT_CAP, *pr, PRIOR_CAP, t["outlier_mp_id"], t["n_outlier_mp"], 2 * FEAT_CAP, B, WINDOW, 0.2,
                                      *[x.data_ptr() for x in self.ins_out], s[1])
        mt = [d["kf_id"], d["kf_pose"], d["n_kf"], Kc, d["mp_id"], d["mp_pos"], d["n_mp"], M, d["obs_mp"], d["obs_kf"], d["obs_flags"], d["n_obs"], N]
        self.map.update_batch(api.MAP_AFTER_INSERT, *mt, s[1], t["outlier_mp_id"], t["n_outlier_mp"], 2 * FEAT_CAP, None, B, s[2])
        self.obs.update_batch(api.MAP_AFTER_INSERT, *tabs, Kc, M, N, s[1], s[2], None, B, s[3])
        oo = [x.data_ptr() for x in self.opt_out]
        self.be.optimize_batch(*tabs, B, K, *oo, s[4])
        self.map.update_batch(api.MAP_AFTER_OPTIMIZE, *mt, s[4], None, None, 0, oo[1], B, s[5])
        self.obs.update_batch(api.MAP_AFTER_OPTIMIZE, *tabs, Kc, M, N, s[4], s[5], oo[0], B, s[6])
        self.trk.clear_links_batch(*self.culled, N, self.n_cleared.data_ptr())
        self.trk.update_from_map(d["kf_id"], d["kf_pose"], d["n_kf"], Kc, d["mp_id"], d["mp_pos"], d["mp_outlier"], d["n_mp"], M)

    def ok(self):
        """how many items the last call mapped with every stage in order"""
        if self.kind == "separate":
            st = torch.stack(self.st, 1)
            return int(((st[:, [0, 1, 2, 3, 4, 5, 6]] == 0).all(1)).sum())
        return int((self.status[:, 0] == 0).sum())


res = {"tool": "tools/mapper_time.py", "build": api.build_id(), "spans_per_form": args.reps, "warm_up_key_frames": WARM,
       "workload": f"window {WINDOW}, {NF} features a key-frame, {STEP} new map points a key-frame, caps {BE_CAPS}, feat_cap {FEAT_CAP}, prior_cap {PRIOR_CAP}", "banks": {}}
for B in args.banks:
    stream = torch.cuda.Stream()
    n_calls = WARM + args.reps + 2
    with torch.cuda.stream(stream):
        trk = api.Tracker(B, 120, 160, FEAT_CAP, 2 * FEAT_CAP, K, stream=stream.cuda_stream)
        forms = {k: Form(B, stream, trk, k, n_calls) for k in ("separate", "mapper", "one in six")}
        ms, mapped = {k: [] for k in forms}, {}
        for rep in range(n_calls):
            for k, f in forms.items():
                f.fill()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f.call()
                torch.cuda.synchronize()
                if rep >= WARM:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
                    mapped.setdefault(k, set()).add(f.ok())
        launches = {"separate": 11, "mapper": forms["mapper"].m.launches_per_call(True), "one in six": forms["one in six"].m.launches_per_call(True)}
    out = {k: dict(median_us=float(np.median(v)) * 1e3, min_us=float(min(v)) * 1e3, max_us=float(max(v)) * 1e3, launches=launches[k], items_mapped_per_call=sorted(mapped[k]))
           for k, v in ms.items()}
    a, b = out["separate"], out["mapper"]
    out["mapper_median_within_separate_spread"] = bool(a["min_us"] <= b["median_us"] <= a["max_us"])
    out["mapper_minus_separate_us_median"] = b["median_us"] - a["median_us"]
    out["clock_mhz"] = float(api.shader_clock_mhz(stream.cuda_stream))
    res["banks"][str(B)] = out
    for k in forms:
        v = out[k]
        print(f"{B:4d} maps  {k:12s} median {v['median_us']:9.1f} us   (min {v['min_us']:.1f}, max {v['max_us']:.1f}; {len(ms[k])} spans, {v['launches']} launches, "
              f"mapped {v['items_mapped_per_call']})", flush=True)
    print(f"{B:4d} maps  mapper - separate: {out['mapper_minus_separate_us_median']:.1f} us (medians); inside the spread of (a): {out['mapper_median_within_separate_spread']}", flush=True)
    del forms, trk
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
