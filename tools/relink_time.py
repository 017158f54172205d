"""Times the re-link at a batch of 64 maps (--batch), by the method of tools/obs_archive_time.py: host clock around spans that end in a synchronise,
warmed up, the forms in alternation, medians with min - max.  Every item is one recorded re-link of the histories of tests/test_relink_ref.py (the one
that moves the most rows) with ITS OWN back end tables, map archive and observation archive, loaded before every span (outside the span):
    parent   the key-frame that follows: ObsArchive.prior_rows_batch -> insert_keyframe_batch -> MapArchive.update_batch -> ObsArchive.update_batch
    new      the nine re-link launches first (plan, stage, back end, map re-link, map update, observation update, first observers, two set_links),
             then the same key-frame
    alone    the nine launches by themselves
Neither form holds myslam_loop_correct_batch or the optimise: the corrector runs before the re-link on the archive's poses and its cost does not depend
on it.  Results go to profiles/relink_time.json (--out names another file).  The tool reports; there is no pass / fail ratio."""
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
import relink_ref as rr  # noqa: E402
from test_gpu_relink_rows import Rows, check_relink, walk_relink  # noqa: E402
from test_whole_map_model import HISTORIES, K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relink_time.json"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
pkg = load_package(); api = pkg.api
B = args.batch

cases = []
for spec in HISTORIES:
    cases += [c for c in rr.replay_rows(pkg.chain, spec, K, record=True)["cases"] if c["next_insert"] is not None and c["plan"]["status"] == rr.DONE]
case = max(cases, key=lambda c: len(walk_relink(pkg.chain, c)["stage"]["rows"]))
items = [case] * B
x = Rows(api, pkg, items)
want = walk_relink(pkg.chain, case)
x.r.stream.wait_stream(torch.cuda.current_stream())
x.relink()                                                                  # warm-up, and what the work is
check_relink(x, x.read(), items, [want] * B, only=(0, B - 1))
x.key_frame()
torch.cuda.synchronize()
plan = case["plan"]
counts = dict(pairs=int(case["count"]), pairs_walked=plan["report"][0], merges=len(plan["merge"]), adopts=len(plan["adopt"]), links=len(plan["links"]),
              moved_rows=len(want["stage"]["rows"]), table_rows_before=sum(len(mp.obs) for mp in case["w_before"].mps.values()),
              table_points_before=len(case["w_before"].mps), archive_points=len(case["a_before"].mp_id), features_of_next_key_frame=len(case["next_insert"].feats))
forms = {"parent: prior_rows + insert + map update + obs update": (False, True), "new: the nine re-link launches, then the same": (True, True),
         "alone: the nine re-link launches": (True, False)}
ms = {k: [] for k in forms}
for rep in range(args.reps + 2):
    for k, (relink, key_frame) in forms.items():
        x.load(items)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if relink:
            x.relink()
        if key_frame:
            x.key_frame()
        torch.cuda.synchronize()
        if rep >= 2:
            ms[k].append((time.perf_counter() - t0) * 1e3)
stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
res = {"workload": f"batch {B}: the re-link of history {case['spec'][:2]} at key-frame {case['cur_kf']} in every slot, each item with its own tables and archives "
                   f"(back end caps {x.be_caps}, feat_cap {rr.FEAT_CAP}, out_cap {rr.OUT_CAP}, row_cap {x.row_cap})",
       "spans": args.reps, "counts": counts, "ms": {k: stat(v) for k, v in ms.items()}}
a, b_ = [res["ms"][k] for k in list(forms)[:2]]
res["added_us_median"] = (b_["median"] - a["median"]) * 1e3
for k, v in res["ms"].items():
    print(f"{k:58s} median {v['median'] * 1e3:9.1f} us   (min {v['min'] * 1e3:.1f}, max {v['max'] * 1e3:.1f}; {args.reps} spans)", flush=True)
print(f"added by the re-link: {res['added_us_median']:.1f} us (medians)")
res["clock_mhz"] = float(api.shader_clock_mhz(x.r.stream.cuda_stream)); res["build"] = api.build_id()
print(f"counts {counts}, clock {res['clock_mhz']:.0f} MHz, build {res['build']}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
