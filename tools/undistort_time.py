"""GPU timing of myslam_undistort_batch (csrc/undistort.hip): one batch of 512 stereo pairs (1024 images) at 1241 x 376 with EuRoC-strength
coefficients, HIP events, against the HBM copy rate of profiles/r03_peaks.json (bytes = one read + one write of every image).
Rows of 1248 bytes (the 1241 columns padded to 16: every output row is stored with dwordx4) and contiguous 1241-byte rows.

    python tools/undistort_time.py [--out profiles/undistort_time.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package(); api = pkg.api
rows, cols, B = 376, 1241, 1024
K = (718.856, 718.856, 607.1928, 185.2157)
D = pkg.synth.EUROC_LIKE_D
copy_gbps = json.load(open(os.path.join(ROOT, "profiles", "r03_peaks.json")))["summary"]["hbm_copy_GBps"]
s = torch.cuda.Stream()
u = api.Undistorter(rows, cols, K, D, stream=s.cuda_stream)
out = {"tool": "tools/undistort_time.py", "build_id": api.build_id(), "images": B, "rows": rows, "cols": cols, "coefficients": list(D),
       "copy_GBps_r03": copy_gbps, "runs": {}}
for step in (1248, 1241):
    stride = rows * step
    src = torch.randint(0, 256, (B * stride,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    run = lambda: u.batch(src.data_ptr(), B, step, stride, dst.data_ptr(), step, stride)
    with torch.cuda.stream(s):
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        N = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(N):
            run()
        e1.record(s); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / N)
    best = min(ms)
    gbps = 2.0 * B * rows * cols / (best * 1e-3) / 1e9
    out["runs"][f"step_{step}"] = {"ms_per_batch": [round(m, 4) for m in ms], "best_ms": round(best, 4), "GBps": round(gbps, 1),
                                    "fraction_of_copy": round(gbps / copy_gbps, 3)}
    del src, dst
print(json.dumps(out))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
