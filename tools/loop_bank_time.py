"""GPU timing of the loop key-frame store bank (csrc/loop_bank.hip): S streams, S in {16, 64, 256}, cap 2400, feat_cap 300, 64 key-frames per stream.

Per shape: the time of one myslam_loop_bank_detect_batch (one launch, every stream a candidate with a full key-frame) and of one
myslam_loop_bank_finish_batch (two launches, every stream stores a full key-frame), and the bytes moved (read + written) over the time; and the time a
caller needs for the same work without the bank — S myslam_loop_store handles with detect_batch(nq = 1) and put_batch(batch = 1, host id) each, on one
stream.  Both are host clocks around enqueued calls that end in a device synchronise, 20 calls (or rounds of S calls) per window, 10 windows per
path, alternating, so that both see the same machine; the best and the worst window are kept.  The bank is cleared before each of its finish
windows (outside the clock): a stream holds 64 key-frames.

    python tools/loop_bank_time.py [--out profiles/loop_bank_time.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package(); api = pkg.api
CAP, FEAT, K = 2400, 300, 64
WINDOWS, N = 10, 20
ITEM_BYTES = CAP * (28 + 32) + FEAT * 4
stream = torch.cuda.Stream()
out = {"tool": "tools/loop_bank_time.py", "build_id": api.build_id(), "cap": CAP, "feat_cap": FEAT, "kfs_per_stream": K,
       "launches_per_finish": api.LoopStoreBank.launches_per_finish(), "windows": WINDOWS, "calls_per_window": N, "item_bytes": ITEM_BYTES,
       "quoted_copy_rate_TBps": 6.3, "shapes": {}}


def window(fn, n=N):
    """ms per call of one window of n calls ended by a synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def stats(ms, moved):
    return {"ms": [round(x, 4) for x in ms], "best_ms": round(min(ms), 4), "worst_ms": round(max(ms), 4), "best_GBps": round(moved / (min(ms) * 1e-3) / 1e9, 1)}


for S in (16, 64, 256):
    with torch.cuda.stream(stream):
        sp = stream.cuda_stream
        bank = api.LoopStoreBank(S, K, CAP, FEAT, stream=sp)
        singles = [api.LoopKeyFrameStore(WINDOWS * N + 8, CAP, FEAT, stream=sp) for _ in range(S)]
        kps = torch.randint(0, 256, (S, CAP, 28), dtype=torch.uint8, device="cuda"); desc = torch.randint(0, 256, (S, CAP, 32), dtype=torch.uint8, device="cuda")
        lm = torch.randint(-1, 1000, (S, FEAT), dtype=torch.int32, device="cuda")
        counts = torch.full((S,), CAP, dtype=torch.int32, device="cuda"); nf = torch.full((S,), FEAT, dtype=torch.int32, device="cuda")
        ones = torch.ones(S, dtype=torch.int32, device="cuda")                  # d_active, and a verify status that is not CONFIRMED
        ids = torch.arange(1, N + 1, dtype=torch.int64, device="cuda")[:, None].repeat(1, S).contiguous()      # call i of a window stores id i + 1
        add = torch.zeros(S, dtype=torch.int32, device="cuda"); fst = torch.zeros(S, dtype=torch.int32, device="cuda")
        reset = torch.ones(S, dtype=torch.int32, device="cuda")
        best = torch.ones(S, dtype=torch.int64, device="cuda"); row = torch.zeros(S, dtype=torch.int32, device="cuda")
        score = torch.full((S,), 0.99, device="cuda"); cnt = torch.zeros(S, dtype=torch.int32, device="cuda")

        def outputs():
            return [torch.zeros((S, CAP, 32), dtype=torch.uint8, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda"),
                    torch.zeros((S, CAP, 28), dtype=torch.uint8, device="cuda"), torch.zeros((S, FEAT), dtype=torch.int32, device="cuda"),
                    torch.zeros(S, dtype=torch.int32, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda")]

        ob, os_ = outputs(), outputs()
        put_no = [0]

        def bank_finish(i):
            bank.finish_batch(ids.data_ptr() + 8 * S * i, ones.data_ptr(), ones.data_ptr(), kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), 0, lm.data_ptr(),
                              nf.data_ptr(), add.data_ptr(), fst.data_ptr())

        def single_puts(i):
            put_no[0] += 1
            kid = np.array([put_no[0]], np.uint64)
            for s in range(S):
                singles[s].put_batch(kid, kps.data_ptr() + s * CAP * 28, desc.data_ptr() + s * CAP * 32, counts.data_ptr() + 4 * s, 0, lm.data_ptr() + s * FEAT * 4,
                                     nf.data_ptr() + 4 * s)

        def bank_detect(i):
            bank.detect_batch(best.data_ptr(), row.data_ptr(), score.data_ptr(), cnt.data_ptr(), *[o.data_ptr() for o in ob])

        def single_detects(i):
            for s in range(S):
                singles[s].detect_batch(best.data_ptr() + 8 * s, score.data_ptr() + 4 * s, cnt.data_ptr() + 4 * s, 1, os_[0].data_ptr() + s * CAP * 32,
                                        os_[1].data_ptr() + 4 * s, os_[2].data_ptr() + s * CAP * 28, os_[3].data_ptr() + s * FEAT * 4, os_[4].data_ptr() + 4 * s,
                                        os_[5].data_ptr() + 4 * s)

        bank_finish(0); single_puts(0); bank_detect(0); single_detects(0)       # warm-up: key-frame id 1 sits at row 0 of every stream and store
        torch.cuda.synchronize()
        same = all(bool((a == b).all()) for a, b in zip(ob, os_)) and bool((ob[5] == 0).all()) and bool((ob[1] == CAP).all()) and bool((fst == api.LOOP_BANK_STORED).all())
        t = {"bank_finish": [], "single_puts": [], "bank_detect": [], "single_detects": []}
        for _ in range(WINDOWS):
            bank.clear_batch(reset.data_ptr())
            t["bank_finish"].append(window(bank_finish))
            stored_ok = bool((fst == api.LOOP_BANK_STORED).all())
            t["single_puts"].append(window(single_puts))
            t["bank_detect"].append(window(bank_detect))
            t["single_detects"].append(window(single_detects))
        torch.cuda.synchronize()
        same = same and stored_ok and all(bool((a == b).all()) for a, b in zip(ob, os_))
    moved = 2 * S * ITEM_BYTES
    shape = {"streams": S, "bytes_moved_per_call": moved, "same_bytes_as_single_stores": same}
    for k, v in t.items():
        shape[k] = stats(v, moved)
    shape["single_over_bank_finish"] = round(shape["single_puts"]["best_ms"] / shape["bank_finish"]["best_ms"], 2)
    shape["single_over_bank_detect"] = round(shape["single_detects"]["best_ms"] / shape["bank_detect"]["best_ms"], 2)
    out["shapes"][f"S{S}"] = shape
    print(f"S{S}", json.dumps(shape), flush=True)
    del bank, singles, kps, desc, lm, ob, os_
print(json.dumps(out))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
