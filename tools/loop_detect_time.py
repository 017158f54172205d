"""Time of LoopKeyFrameStore.detect_batch (myslam_loop_detect_batch, csrc/loop_store.hip) against a plain device-to-device copy of the same number of
bytes on the same device, alternating A B A B:
  A  detect_batch: 64 key-frames of 3000 rows stored (cap 4096, feat_cap 512, 512 landmark entries each), nq items, every one a candidate, the
     key-frames named round robin;
  B  one torch copy_ of a contiguous uint8 buffer of nq x (3000 x 60 + 512 x 4) bytes — what the gather moves, without its dependent reads
     (score, count, the id search, the row count) and in one piece instead of 3 nq pieces.
nq = 1, 8, 64, 512.  HIP events around windows of back-to-back launches on one stream (each window >= ~50 ms after warm-up), the median window per
launch; both pairs of passes are kept so that the spread shows.  The aim is A <= 2 B at nq >= 64; nothing is asserted.  Note for reading the
numbers: A's source is the 64-key-frame store (16 MB, cache resident) while B's source is as large as its destination.
Writes profiles/loop_detect_time.json.

    python tools/loop_detect_time.py [--out profiles/loop_detect_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one HIP runtime for the process: before the library)

from __graft_entry__ import load_package  # noqa: E402

CAP, FEAT, KFS, ROWS = 4096, 512, 64, 3000
ITEM_BYTES = ROWS * 60 + FEAT * 4


def windows(launch, n_windows=5, min_ms=50.0, warm=20):
    """median over n_windows of (event time of `reps` back-to-back launches) / reps, in microseconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        launch()
    e0.record()
    for _ in range(50):
        launch()
    e1.record(); e1.synchronize()
    reps = int(min(20000, max(50, min_ms / max(e0.elapsed_time(e1) / 50, 1e-4))))
    out = []
    for _ in range(n_windows):
        e0.record()
        for _ in range(reps):
            launch()
        e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out)), "launches_per_window": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_detect_time.json"))
    a = ap.parse_args()
    api = load_package().api
    assert api.device_count() >= 1, "no HIP device: this tool measures on the GPU and has no other path"
    dev = "cuda"
    store = api.LoopKeyFrameStore(KFS, CAP, FEAT)
    g = torch.Generator(device=dev); g.manual_seed(1)
    for k0 in range(0, KFS, 16):                         # 16 key-frames per put keeps the staging small
        kps = torch.randint(0, 256, (16, CAP, 28), dtype=torch.uint8, device=dev, generator=g)
        desc = torch.randint(0, 256, (16, CAP, 32), dtype=torch.uint8, device=dev, generator=g)
        lm = torch.randint(-1, 4096, (16, FEAT), dtype=torch.int32, device=dev, generator=g)
        cnt = torch.full((16,), ROWS, dtype=torch.int32, device=dev); nf = torch.full((16,), FEAT, dtype=torch.int32, device=dev)
        store.put_batch(np.arange(k0, k0 + 16, dtype=np.uint64) * 5 + 2, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), 0, lm.data_ptr(), nf.data_ptr())
        torch.cuda.synchronize()
    rows = []
    for nq in a.nq:
        best = torch.from_numpy(((np.arange(nq) % KFS) * 5 + 2).astype(np.int64)).to(dev)
        score = torch.full((nq,), 0.99, dtype=torch.float32, device=dev); cnt = torch.ones(nq, dtype=torch.int32, device=dev)
        o_desc = torch.zeros(nq, CAP, 32, dtype=torch.uint8, device=dev); o_pyr = torch.zeros(nq, CAP, 28, dtype=torch.uint8, device=dev)
        o_lm = torch.zeros(nq, FEAT, dtype=torch.int32, device=dev)
        o_n, o_slot, o_st = (torch.zeros(nq, dtype=torch.int32, device=dev) for _ in range(3))
        src = torch.randint(0, 256, (nq * ITEM_BYTES,), dtype=torch.uint8, device=dev, generator=g); dst = torch.zeros_like(src)

        def gather():
            store.detect_batch(best.data_ptr(), score.data_ptr(), cnt.data_ptr(), nq, o_desc.data_ptr(), o_n.data_ptr(), o_pyr.data_ptr(), o_lm.data_ptr(),
                               o_slot.data_ptr(), o_st.data_ptr())

        def copy():
            dst.copy_(src)

        gather(); torch.cuda.synchronize()
        assert (o_st == 0).all() and (o_n == ROWS).all(), "not every item was a candidate: the timed launches would not move the bytes they are charged"
        A, B = [], []
        for _ in range(2):                                # A B A B
            A.append(windows(gather)); B.append(windows(copy))
        ratio = [x["median_us"] / y["median_us"] for x, y in zip(A, B)]
        bytes_moved = 2 * nq * ITEM_BYTES
        row = {"nq": nq, "bytes_read_plus_written": bytes_moved, "detect_us": A, "copy_us": B, "detect_over_copy": ratio,
               "detect_GBps": [bytes_moved / x["median_us"] / 1e3 for x in A], "copy_GBps": [bytes_moved / y["median_us"] / 1e3 for y in B]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del o_desc, o_pyr, src, dst
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/loop_detect_time.py", "cap": CAP, "feat_cap": FEAT, "key_frames": KFS, "rows_per_key_frame": ROWS,
                   "item_bytes": ITEM_BYTES, "device": torch.cuda.get_device_name(0), "aim": "detect_over_copy <= 2 at nq >= 64", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
