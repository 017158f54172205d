#!/usr/bin/env python3
"""bench.py — stereo frames/s of the per-frame dense path on MI355X (BASELINE.json metric).

A "step" = one pass of the hot path over one batch (default 512) of synthetic 1241x376 stereo pairs resident in HBM:
  ORB DetectAndCompute (2000 features) on left+right -> L/R 256-bit Hamming match -> stereo triangulation
  -> DeepLCD descriptor of the left image -> cosine scan of the key-frame database -> local-BA block build
  (one DISTINCT 10 KF x 300 landmark window per frame).  [BASELINE.json configs[3]; --workload orb_match = configs[1]]

One process per GPU.  `python bench.py --gpus N` launches its N ranks itself when it is not already running under
torch.distributed.run (which works as before: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment).  Frames shard
across ranks (stream r on rank r, no data-path collective); the loop database is sharded by key-frame id range and the only
exchange is an all-gather of the query descriptors and of the 16-byte per-shard candidate records (RCCL).

Passes (all after the warm-up, each bracketed by barrier + synchronize):
  1. the TIMED region: K steps, per-kernel event profiling OFF            -> value, ms_per_step
  2. a profiled pass: the same K steps with a HIP event pair around every launch (on the launch's stream) -> roofline
  3. (full workload) K steps with the OptimizeActiveMap solve on 1 frame in 6 (the reference's key-frame cadence) -> full_solve_cadence6
A plain run (`--gpus N --steps K --warmup W`) does pass 1 only: set-up, warm-up, the K timed steps, the line.  Everything else (the repeat regions and the
clock probes, passes 2 onward, the rooflines, the oracle parity sample, the CPU baseline, the live-stream children) runs under --full.
--dump-outputs DIR writes what the last timed step computed (bench/dump.py).
Prints ONE JSON line (rank 0).  PyTorch is used for device memory, streams and torch.distributed only.

This file is the entry point and the timed schedule (set-up, the step functions, passes 1-6, the verification steps, the JSON line).  Everything
else lives in the package bench/ (round 5 split, no behaviour change): args.py (command line), config.py (constants, algorithmic bytes),
runtime.py (self-launch, host cores), profiles.py (committed counter / peak files), report.py (roofline objects), passes_multirank.py (the
loop-database exchange stage by stage), passes_stream_mode.py (live-stream operating points), cpu_baseline.py and parity_sample.py (the two
oracle legs: the only importers of oracle/ outside tests/ and smoke()).
"""
import argparse
import glob
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np

# The ROCm runtime multiplexes HIP streams onto GPU_MAX_HW_QUEUES (default 4) HSA hardware queues, and streams that share a queue
# serialise — a host->device copy on one of them stalls the kernels of the other (measured: the streamed pass ran at copy + compute
# instead of max(copy, compute)).  The default schedule uses 6 streams (two extractor handles, match + BA build, DeepLCD + DB scan, two
# input-copy streams: the left and the right images of a streamed step cross PCIe as two concurrent copies): one hardware queue each
# (4, 5 and 6 queues measure the same on the resident pass).  A runtime setting of the application, stated in the JSON (config.hip_hw_queues); the library reads no
# environment variable.  Must be set before the HIP runtime initialises (i.e. before `import torch`).
def _ranks_wanted():
    if "WORLD_SIZE" in os.environ:
        return int(os.environ["WORLD_SIZE"])
    for i, a in enumerate(sys.argv):
        if a == "--gpus" and i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit():
            return int(sys.argv[i + 1])
        if a.startswith("--gpus=") and a[7:].isdigit():
            return int(a[7:])
    return 1


# N > 1: torch's process group brings one more stream (the collectives' own) — one more queue
def _small_batch():
    for i, a in enumerate(sys.argv):
        if a == "--pairs" and i + 1 < len(sys.argv) and sys.argv[i + 1].isdigit():
            return int(sys.argv[i + 1]) <= 64
    return False


# N > 1: torch's process group brings one more stream (the collectives' own) — one more queue; small batches run on up to 16 lanes, and
# lanes that share a hardware queue serialise (8 pairs per step, 16 lanes: 17.1 k frames/s on 8 queues, 19.0 k on 16, 26.5 k on 24)
HW_QUEUES = os.environ.setdefault("GPU_MAX_HW_QUEUES", ("24" if _small_batch() else "6") if _ranks_wanted() == 1 else "7")

# Kernel arguments in device memory instead of host-visible memory (round 6): every block of every kernel starts with scalar loads out of its argument block, and the FAST
# kernel's blocks live ~10 us of which ~2 are that head (DESIGN_APPENDIX.md section 10).  Same-box A/B: 6.484 / 6.447 / 6.449 -> 6.428 / 6.419 / 6.432 ms per step.  Like the
# queue count a runtime setting of the APPLICATION, stated in the line (config.hip_dev_kernarg); the library reads no environment variable.
DEV_KERNARG = os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from bench.args import parse  # noqa: E402
from bench.config import H, SYMBOL, W  # noqa: E402
from bench.cpu_baseline import cpu_baseline  # noqa: E402
from bench.dump import sample_frames, write as write_outputs  # noqa: E402
from bench.parity_sample import parity_sample  # noqa: E402
from bench.report import ba_solve_roofline, rooflines  # noqa: E402
from bench.passes_multirank import db_exchange  # noqa: E402
from bench.passes_stream_mode import stream_mode_sweep  # noqa: E402
from bench.runtime import masked_stream, self_launch  # noqa: E402

def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)
    # The live-stream operating points are measured by child processes (their own GPU_MAX_HW_QUEUES) FIRST, before this process creates its GPU context: a
    # child that ran beside the parent's idle context — its hardware queues stay mapped — measured 10.1 k frames/s at 1 pair x 16 lanes where the same command
    # alone on the chip measures 12.3 k (tools/ab_stream_mode.sh).
    stream_mode = None
    if int(os.environ.get("WORLD_SIZE", "1")) == 1 and args.stream_mode and not args.no_extra_passes and args.workload in ("full", "orb_match_lcd") and not args.stream_mode_late:
        stream_mode = stream_mode_sweep(args)
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    via_cpu = args.backend == "gloo"
    if via_cpu:
        local_rank = 0
    assert args.gpus == world, f"--gpus {args.gpus} but WORLD_SIZE {world} (under torch.distributed.run pass --gpus = --nproc-per-node)"
    rccl_ranks = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        assert via_cpu or torch.cuda.device_count() > local_rank, \
            f"rank {rank}: {torch.cuda.device_count()} visible GPU(s) but LOCAL_RANK {local_rank} (one GPU per rank; --backend gloo shares GPU 0)"
        torch.cuda.set_device(local_rank)
        if via_cpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        one = torch.ones(1, dtype=torch.int32, device="cpu" if via_cpu else torch.device("cuda", local_rank))
        dist.all_reduce(one)                                     # the ranks the collective library actually connected
        rccl_ranks = int(one.item())
        assert rccl_ranks == world
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank if world > 1 else 0)

    pkg = load_package()
    api, synth = pkg.api, pkg.synth
    assert api.device_count() >= 1
    if args.workload == "latency":
        assert world == 1
        from tools import latency_b1
        print(json.dumps(latency_b1.run(api, synth, with_oracle=not args.no_cpu_baseline)))
        return
    # the four-stream schedule keeps its main chain on the legacy NULL stream: measured, its launches cost the host 0.63 ms per step there and
    # 1.02 ms on a created stream (8 pairs per step; tools/ab_streams.sh) — the lanes of the small-batch mode bring their own streams
    if args.created_main_stream:
        torch.cuda.set_stream(torch.cuda.Stream())
    main_stream = torch.cuda.current_stream()
    stream = main_stream.cuda_stream
    # the LCD -> DB -> BA chain only reads the input images: it runs beside the ORB chain on its own stream
    side_stream = (masked_stream(args.side_cus) if args.side_cus > 0 else torch.cuda.Stream()) if args.streams == 2 else main_stream
    stream2 = side_stream.cuda_stream
    P = args.pairs
    K = synth.KITTI00
    Kt = (K["fx"], K["fy"], K["cx"], K["cy"])

    # ---- inputs resident in HBM before the timed region ----
    frames = synth.stereo_batch(P, stream_id=rank, n_rect=args.scene_rects)   # [P, 2, H, W]
    imgs = np.concatenate([frames[:, 0], frames[:, 1]], axis=0)         # all left images, then all right images
    d_imgs = torch.from_numpy(imgs).to(dev)
    cur = {"imgs": d_imgs}              # the device buffer the steps read their images from (the streamed pass swaps it per step)
    ext = api.ORBextractor(2000, stream=stream)
    cap = ext.max_keypoints()
    S = args.orb_split
    assert (2 * P) % S == 0
    orb_streams = [torch.cuda.Stream() for _ in range(S - 1)]
    orb_exts = [api.ORBextractor(2000, stream=st.cuda_stream) for st in orb_streams]
    for e in [ext] + orb_exts:
        e.set_option(e.OPT_INTERNAL_STREAM, args.orb_internal_stream)
        e.set_option(e.OPT_FAST_MODE, args.fast_mode)
        e.set_option(e.OPT_COPY_INPUT, args.orb_copy_input)
        e.set_option(e.OPT_BLUR_MFMA, args.blur_mfma)
        e.set_option(e.OPT_SIDE_BLOCKS_PER_CU, args.side_blocks_per_cu)
    NB = 2 if args.pipeline else 1          # pipeline: extractor outputs are double-buffered (step k+1 extracts while step k is matched)
    d_kps_b = [torch.zeros(2 * P * cap * 28, dtype=torch.uint8, device=dev) for _ in range(NB)]
    d_desc_b = [torch.zeros(2 * P * cap * 32, dtype=torch.uint8, device=dev) for _ in range(NB)]
    d_cnt_b = [torch.zeros(2 * P, dtype=torch.int32, device=dev) for _ in range(NB)]
    d_stat_b = [torch.zeros(2 * P, dtype=torch.int32, device=dev) for _ in range(NB)]
    d_kps, d_desc, d_cnt, d_stat = d_kps_b[0], d_desc_b[0], d_cnt_b[0], d_stat_b[0]
    d_midx = torch.zeros(P * cap, dtype=torch.int32, device=dev)
    d_mdist = torch.zeros(P * cap, dtype=torch.int32, device=dev)
    d_xyz = torch.zeros(P * cap * 3, dtype=torch.float64, device=dev)
    d_ok = torch.zeros(P * cap, dtype=torch.uint8, device=dev)
    use_lcd = args.workload != "orb_match"
    use_ba = args.workload in ("full", "full_solve")
    use_solve = args.workload == "full_solve"
    # --emulate-world N (round 6): ONE process, no collective — this rank does what a rank of an N-GPU job does per step: it scans N P queries (its own P, as
    # the all-gather would deliver them, + (N - 1) P resident ones) against a 6 250-row shard and merges N candidate sets (its own + N - 1 resident ones).
    # What an N-GPU run adds on top are the two all-gathers only (DESIGN.md section 4 keeps those modelled).
    emu = args.emulate_world if (args.emulate_world > 1 and world == 1) else 0
    shards = world if world > 1 else (emu or 1)
    n_db_local = args.db or (10000 if shards == 1 else 6250)
    db_np = None
    if use_lcd:
        lcd = api.DeepLCD(synth.calc_weights(), stream=stream2)
        # the DeepLCD chain in `lcd_split` parts on as many handles / streams (part 0 on the side stream): every stream of the schedule is
        # busy for about the whole step, and the side stream's chain was the longest — two half-length chains overlap better (+0.9 %)
        lcd_parts = []
        if args.lcd_split > 1 and P % args.lcd_split == 0 and args.streams == 2:
            for _ in range(args.lcd_split - 1):
                st_ = torch.cuda.Stream()
                lcd_parts.append((api.DeepLCD(synth.calc_weights(), stream=st_.cuda_stream), st_, torch.cuda.Event()))
            ev_lfork = torch.cuda.Event()
        if args.lcd_skip:
            lcd.set_option(lcd.OPT_SKIP_KERNELS, args.lcd_skip)
        d_descr = torch.zeros(P, 1064, device=dev)
        db_np = synth.lcd_database(n_db_local, seed=0xDB + rank)
        D = api.LoopDatabase(n_db_local, stream=stream2)
        ids = np.arange(rank * n_db_local, (rank + 1) * n_db_local, dtype=np.uint64)     # contiguous id range per shard
        t_db = torch.from_numpy(db_np).to(dev)
        D.append_batch(ids, t_db.data_ptr(), n_db_local)
        NQ = P * shards
        cur_ids = np.full(NQ, shards * n_db_local + 20, np.uint64)
        d_allq = torch.zeros(NQ, 1064, device=dev)
        d_best = torch.zeros(NQ, dtype=torch.int64, device=dev)
        d_max = torch.zeros(NQ, device=dev); d_dbcnt = torch.zeros(NQ, dtype=torch.int32, device=dev)
        d_cand = torch.zeros(NQ * 16, dtype=torch.uint8, device=dev)
        if world > 1:
            pkg.sharded_db.check_shard_order(int(ids[0]), int(ids[-1]), world, via_cpu=via_cpu, device=dev)
        if emu:
            # the other ranks' queries: unit vectors near rows of THEIR shards' kind (resident; a real job receives them by all-gather every step)
            oq = synth.lcd_database(NQ - P, seed=0xE0)
            d_allq[P:].copy_(torch.from_numpy(oq).to(dev))
            # the other ranks' candidate records: what their shards would answer — here the answers of this shard to shifted queries, ids moved into their ranges
            d_gath = torch.zeros(emu, NQ * 16, dtype=torch.uint8, device=dev)
            D.query_batch_sharded(d_allq.data_ptr(), cur_ids, NQ, d_cand.data_ptr()); torch.cuda.synchronize()
            for r_ in range(1, emu):
                d_gath[r_].copy_(d_cand)
    ba_w = None
    if use_ba:
        ba_w, _ = synth.ba_windows(P, seed0=0xBA + 100000 * rank)        # P DISTINCT windows (10 KF x 300 MP, ~2950 edges each)
        maxP, maxL, maxE = ba_w[0].shape[1], ba_w[1].shape[1], ba_w[2].shape[1]
        b_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in ba_w]
        b_out = [torch.zeros(P, n, dtype=torch.float64, device=dev) for n in (maxP * 36, maxL * 9, maxE * 18, maxP * 6, maxL * 3, maxE)]
        # the solve updates poses/points in place: every step starts from the pristine windows
        s_poses, s_pts = b_in[0].clone(), b_in[1].clone()
        s_echi = torch.zeros(P, maxE, dtype=torch.float64, device=dev); s_out = torch.zeros(P, maxE, dtype=torch.uint8, device=dev)
        s_rd = torch.zeros(P, dtype=torch.int32, device=dev); s_no = torch.zeros(P, dtype=torch.int32, device=dev)
        s_st = torch.zeros(P, dtype=torch.int32, device=dev)

        # The solve has its own stream (round 5): Backend::OptimizeActiveMap runs on the Backend thread, beside LoopClosing's DeepLCD / DB chain
        # (src/backend.cpp:36-49, src/loopclosing.cpp:66-81), and needs nothing from it.  Behind the side chain it made that chain the step's
        # longest (+0.75 ms per step for 86 windows of 1.1 ms each); on its own stream the step pays only for the CUs the solve's blocks hold.
        solve_stream = torch.cuda.Stream() if (args.solve_stream == "own" and args.streams == 2) else side_stream
        s_hpl = torch.zeros(P, maxE * 18, dtype=torch.float64, device=dev) if solve_stream is not side_stream else b_out[2]     # the solve's scratch (the build writes b_out[2] at the same time)

        def solve(nwin=P):   # Backend::OptimizeActiveMap solve stage: rounds of optimize(10) + outlier flags (backend.cpp:208-243)
            with torch.cuda.stream(solve_stream):
                s_poses[:nwin].copy_(b_in[0][:nwin]); s_pts[:nwin].copy_(b_in[1][:nwin])
                api.ba_optimize_active_map_batch(s_poses.data_ptr(), s_pts.data_ptr(), *[t.data_ptr() for t in b_in[2:]], nwin, maxP, maxL, maxE, Kt,
                                                 5.991, 5.991, 5, 10, s_hpl.data_ptr(), s_echi.data_ptr(), s_out.data_ptr(), s_rd.data_ptr(),
                                                 s_no.data_ptr(), s_st.data_ptr(), solve_stream.cuda_stream)
    solve_windows = [P if use_solve else 0]          # windows the side chain also SOLVES per step (pass 3 sets ceil(P / 6))

    skip = set(args.side_skip.split(",")) if args.side_skip else set()      # diagnostic: the marginal cost of the side chain's parts
    grow = [False, 0, [], None]                            # pass "db_grow": [on, next key-frame id, the appended row blocks (kept for the check after the pass)]

    def side_chain(with_ba=True):
        if use_ba and "ba" not in skip and solve_windows[0] and solve_stream is not side_stream:
            solve_stream.wait_stream(side_stream)      # starts with the step (the side stream has just waited for the step's start event), runs beside the chain below
            solve(solve_windows[0])
        if use_lcd and "lcd" not in skip:
            if lcd_parts:
                n_part = P // (len(lcd_parts) + 1)
                ev_lfork.record(side_stream)
                for i, (h_, st_, ev_) in enumerate(lcd_parts):
                    st_.wait_event(ev_lfork)
                    h_.describe_batch(cur["imgs"].data_ptr() + (i + 1) * n_part * H * W, n_part, H, W, W, H * W,
                                      d_descr.data_ptr() + (i + 1) * n_part * 1064 * 4, blur_in_place=False)
                    ev_.record(st_)
                lcd.describe_batch(cur["imgs"].data_ptr(), n_part, H, W, W, H * W, d_descr.data_ptr(), blur_in_place=False)
                for _, _, ev_ in lcd_parts:
                    side_stream.wait_event(ev_)
            else:
                lcd.describe_batch(cur["imgs"].data_ptr(), P, H, W, W, H * W, d_descr.data_ptr(), blur_in_place=False)
        if use_lcd and "db" not in skip:
            if emu:             # one rank of an N-rank job without the collectives: own queries into the gathered block, N P queries against the shard, merge of N sets
                d_allq[:P].copy_(d_descr)
                D.query_batch_sharded(d_allq.data_ptr(), cur_ids, NQ, d_gath.data_ptr())                 # this shard's records = set 0 of the gathered block
                api.lcd_merge_candidates_device(d_gath.data_ptr(), emu, NQ, d_best.data_ptr(), d_max.data_ptr(), d_dbcnt.data_ptr(), stream2)
            elif world > 1:     # every shard scores every rank's queries; the 16-byte candidate records are merged after an all-gather
                if via_cpu:
                    h_all = torch.empty(d_allq.shape, dtype=d_allq.dtype)
                    dist.all_gather_into_tensor(h_all, d_descr.cpu())
                    d_allq.copy_(h_all)
                else:
                    dist.all_gather_into_tensor(d_allq, d_descr)
                D.query_batch_sharded(d_allq.data_ptr(), cur_ids, NQ, d_cand.data_ptr())
                pkg.sharded_db.exchange_and_merge(d_cand, world, d_best, d_max, d_dbcnt, via_cpu=via_cpu)
            else:
                D.query_batch(d_descr.data_ptr(), cur_ids, NQ, d_best.data_ptr(), d_max.data_ptr(), d_dbcnt.data_ptr())
            if grow[0]:         # LoopClosing::AddToDatabase (src/loopclosing.cpp:651-659) after DetectLoop: the step's key-frames (1 frame in 6) join the database, on this stream, no host wait
                nkf = (P + 5) // 6
                # (rows of a pool allocated before the pass: a fresh tensor per step made torch's caching allocator call hipMalloc inside the timed region —
                # a device-synchronising call of milliseconds, bimodal 6.5 / 9 ms per step in a 20-step region)
                d_kf = grow[3][len(grow[2]) % grow[3].shape[0]]
                d_kf.copy_(d_descr[::6][:nkf])
                kf_ids = np.arange(grow[1], grow[1] + nkf, dtype=np.uint64)
                D.append_batch_async(kf_ids, d_kf.data_ptr(), nkf, stream2)
                grow[1] += nkf; grow[2].append(d_kf)
                cur_ids[:] = grow[1] + 20 + P              # the next step's frames: ids beyond everything in the database (no cut-off), as in the other passes
        if use_ba and "ba" not in skip:
            if with_ba or solve_windows[0]:
                api.ba_build_batch(*[t.data_ptr() for t in b_in], P, maxP, maxL, maxE, Kt, 5.991, *[t.data_ptr() for t in b_out], stream2)
            if solve_windows[0] and solve_stream is side_stream:
                solve(solve_windows[0])

    ba_on_match = [False]
    step_no = [0]           # steps issued so far: step k writes extractor output buffer k % NB
    if args.pipeline:
        ba_on_match[0] = args.ba_stream == "match" and use_ba
        # two extractor handles take turns: handle A (left images, main stream) and handle B (right images, its own stream) each wait
        # for the other's FAST stage, so a FAST launch never runs beside the other FAST launch but under the other handle's oct-tree /
        # descriptor launches; match + triangulation of step k run on a third stream once both handles are done with step k, while the
        # handles already extract step k+1 into the other output buffer
        exts = [ext] + orb_exts
        sX, sM = [main_stream] + orb_streams, (masked_stream(args.match_cus) if args.match_cus > 0 else torch.cuda.Stream())
        G = 2 * P // S
        ev_fast = [torch.cuda.Event() for _ in range(S)]
        ev_done = [[torch.cuda.Event() for _ in range(S)] for _ in range(NB)]
        ev_match = [torch.cuda.Event() for _ in range(NB)]
        ev_start = torch.cuda.Event()
        for e in ev_fast + [x for pr in ev_done for x in pr] + ev_match + [ev_start]:
            e.record(main_stream)                       # creates the hipEvent_t behind the torch event
        for i, e in enumerate(exts):
            e.set_fast_event(ev_fast[i].cuda_event)
            if args.pipeline == 1:      # gate inside the call: only the FAST stages take turns (ring), the pyramids are not held back
                e.set_fast_gate(ev_fast[(i - 1) % S].cuda_event)

        def step():
            p = step_no[0] % NB
            step_no[0] += 1
            kps, desc, cnt, stat = d_kps_b[p], d_desc_b[p], d_cnt_b[p], d_stat_b[p]
            for i, e in enumerate(exts):
                if args.pipeline == 2:
                    sX[i].wait_event(ev_fast[(i - 1) % S])      # the previous handle's FAST (whole call held back)
                sX[i].wait_event(ev_match[p])                   # buffer p was last read by the match of step k - 2
                if i == 0:
                    ev_start.record(sX[0])
                o = i * G
                e.detect_and_compute_batch(cur["imgs"].data_ptr() + o * H * W, G, H, W, W, H * W, kps.data_ptr() + o * cap * 28,
                                           desc.data_ptr() + o * cap * 32, cnt.data_ptr() + 4 * o, stat.data_ptr() + 4 * o, cap)
                ev_done[p][i].record(sX[i])
            for i in range(S):
                sM.wait_event(ev_done[p][i])
            api.hamming_match_batch(desc.data_ptr(), cnt.data_ptr(), desc.data_ptr() + P * cap * 32, cnt.data_ptr() + 4 * P,
                                    P, cap, d_midx.data_ptr(), d_mdist.data_ptr(), sM.cuda_stream)
            api.triangulate_stereo_batch(kps.data_ptr(), kps.data_ptr() + P * cap * 28, d_midx.data_ptr(), cnt.data_ptr(), P, cap,
                                         Kt, K["bf"] / K["fx"], d_xyz.data_ptr(), d_ok.data_ptr(), sM.cuda_stream)
            ev_match[p].record(sM)
            if ba_on_match[0] and "ba" not in skip and not solve_windows[0]:
                api.ba_build_batch(*[t.data_ptr() for t in b_in], P, maxP, maxL, maxE, Kt, 5.991, *[t.data_ptr() for t in b_out], sM.cuda_stream)
            side_stream.wait_event(ev_start)            # the LCD / DB / BA chain of step k starts with step k
            with torch.cuda.stream(side_stream):
                side_chain(with_ba=not ba_on_match[0])

    def step_joined():
        if S == 1:
            ext.detect_and_compute_batch(cur["imgs"].data_ptr(), 2 * P, H, W, W, H * W, d_kps.data_ptr(), d_desc.data_ptr(),
                                         d_cnt.data_ptr(), d_stat.data_ptr(), cap)
        else:               # S equal groups of images, group 0 on the main stream
            G = 2 * P // S
            for st in orb_streams:
                st.wait_stream(main_stream)
            for gi, e in enumerate([ext] + orb_exts):
                o = gi * G
                e.detect_and_compute_batch(cur["imgs"].data_ptr() + o * H * W, G, H, W, W, H * W, d_kps.data_ptr() + o * cap * 28,
                                           d_desc.data_ptr() + o * cap * 32, d_cnt.data_ptr() + 4 * o, d_stat.data_ptr() + 4 * o, cap)
            for st in orb_streams:
                main_stream.wait_stream(st)
        api.hamming_match_batch(d_desc.data_ptr(), d_cnt.data_ptr(), d_desc.data_ptr() + P * cap * 32, d_cnt.data_ptr() + 4 * P,
                                P, cap, d_midx.data_ptr(), d_mdist.data_ptr(), stream)
        api.triangulate_stereo_batch(d_kps.data_ptr(), d_kps.data_ptr() + P * cap * 28, d_midx.data_ptr(), d_cnt.data_ptr(), P, cap,
                                     Kt, K["bf"] / K["fx"], d_xyz.data_ptr(), d_ok.data_ptr(), stream)
        if side_stream is not main_stream:
            side_stream.wait_stream(main_stream)            # a joined step starts behind everything issued before it (found by --verify on two
        with torch.cuda.stream(side_stream):                # ranks sharing a GPU: the zeroing of the outputs raced with this chain)
            side_chain()
        if side_stream is not main_stream:
            main_stream.wait_stream(side_stream)            # a step is complete when both chains are

    if not args.pipeline:
        step = step_joined

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    host_ms = [0.0]
    rank_dts = []           # multi-rank runs: every rank's wall time of the last timed() call ...
    rank_own = []           # ... and the time at which its own device had finished, before the closing barrier

    def timed(n, fn=None, lead=3):
        """n steps bracketed by barrier + synchronize on both sides; the slowest rank's wall time.  `lead` untimed steps of the same kind run straight before the
        opening barrier (the secondary passes: their set-up leaves the chip idle, and after an idle gap the first ~0.1 s run 2 - 3 % slow —
        profiles/r06_ab_warmup_gap.json; the timed region itself follows the contract's W warm-up steps and passes lead=0).  host_ms[0] = CPU time the launches of
        one step took: the enqueue loop's time per step over its first 8 steps — after ~10 steps of 512 pairs the runtime's queues are
        full and the loop runs at the DEVICE's pace (back-pressure: 3 ms per step over 200 steps, 0.2 ms over the first 8), which is not
        a cost of launching"""
        fn = fn or step
        for _ in range(lead):
            fn()
        barrier()
        t0 = time.perf_counter()
        n_host = min(n, 8)
        for i in range(n):
            fn()
            if i + 1 == n_host:
                host_ms[0] = (time.perf_counter() - t0) / n_host * 1e3
        t_own = 0.0
        if world > 1:                       # when THIS rank's device finished its own work, before it waits for the others
            torch.cuda.synchronize()
            t_own = time.perf_counter() - t0
        barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            # every rank's wall time up to the closing barrier (nearly equal by construction), the time at which its own device was done, and
            # the slowest one, which is the job's time
            t = torch.tensor([dt, t_own], dtype=torch.float64, device="cpu" if via_cpu else dev)
            allt = torch.empty(2 * world, dtype=torch.float64, device=t.device)
            dist.all_gather_into_tensor(allt, t)
            v = [float(x) for x in allt.cpu()]
            rank_dts[:] = v[0::2]; rank_own[:] = v[1::2]
            dt = max(rank_dts)
        return dt

    # Two untimed steps for the run's own checks (capacity overflow, key-points per image).  The W warm-up steps of the contract run further down, STRAIGHT before
    # the timed region (build v68): up to v67 they ran here, and the checks' host synchronisations, the lanes' set-up and the clock probe (a one-wave kernel on an
    # idle chip) lay between them and the region — after that idle gap the chip took ~0.1 s to return to its loaded state, 2 - 3 % of a 20-step region
    # (tools/ab_warmup_gap.sh: first region 6.40 / 6.36 / 6.54 ms per step against 6.22 / 6.18 / 6.38 for the identical regions that followed it).
    for _ in range(args.warmup if args.gap_before_timed else 2):
        step()
    barrier()
    assert all(int(t.abs().sum()) == 0 for t in d_stat_b), "ORB capacity overflow"
    n_kp = d_cnt.float().mean().item()

    # ---- small batches: LANES.  A step of a few frames is a latency-bound chain of ~38 dependent launches (0.86 ms at 8 pairs on one
    # stream, 0.53 ms host-bound on four).  Measured on ROCm 7.2: a HIP graph recorded from ONE stream replays for ~0.03 ms of host time,
    # one recorded across streams for 0.36-0.75 ms (no better than launching eagerly).  So the step is recorded per lane on a single
    # stream — one extractor handle for the 2P images, match, triangulation, DeepLCD, database scan, BA build — and L lanes (own handles,
    # buffers and stream each: the analogue of L cameras) replay their graphs concurrently: step k runs on lane k % L.
    step_eager = step
    lanes = []
    can_graph = world == 1
    use_graph = can_graph and (args.graph == 1 or (args.graph < 0 and P <= 64))
    n_lanes = args.lanes if args.lanes > 0 else (16 if P <= 32 else 8 if P <= 64 else 4)       # measured: 32 pairs 70.5 k on 16 lanes, 68.1 k on 8; 64 pairs 72.4 k on 8 or 12, 71.4 k on 16

    def build_lane():
        st = torch.cuda.Stream(); s_ = st.cuda_stream
        ln = {"stream": st, "ext": api.ORBextractor(2000, stream=s_)}
        ln["ext"].set_option(ln["ext"].OPT_INTERNAL_STREAM, 0); ln["ext"].set_option(ln["ext"].OPT_FAST_MODE, args.fast_mode)
        ln["ext"].set_option(ln["ext"].OPT_COPY_INPUT, args.orb_copy_input); ln["ext"].set_option(ln["ext"].OPT_BLUR_MFMA, args.blur_mfma)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
        o = {"kps": z(2 * P * cap * 28, torch.uint8), "desc": z(2 * P * cap * 32, torch.uint8), "cnt": z(2 * P, torch.int32), "stat": z(2 * P, torch.int32),
             "midx": z(P * cap, torch.int32), "mdist": z(P * cap, torch.int32), "xyz": z(P * cap * 3, torch.float64), "ok": z(P * cap, torch.uint8)}
        if use_lcd:
            ln["lcd"] = api.DeepLCD(synth.calc_weights(), stream=s_)
            ln["D"] = D.context(s_)                                       # ONE database for all lanes (LoopClosing::_mvDatabase is one std::map per process, loopclosing.h:120): a query context per lane
            o.update({"descr": torch.zeros(P, 1064, device=dev), "best": z(P, torch.int64), "max": z(P, torch.float32), "dbcnt": z(P, torch.int32)})
        if use_ba:
            o["ba"] = [torch.zeros(P, n, dtype=torch.float64, device=dev) for n in (maxP * 36, maxL * 9, maxE * 18, maxP * 6, maxL * 3, maxE)]
        ln["o"] = o

        def body():
            ln["ext"].detect_and_compute_batch(d_imgs.data_ptr(), 2 * P, H, W, W, H * W, o["kps"].data_ptr(), o["desc"].data_ptr(), o["cnt"].data_ptr(),
                                               o["stat"].data_ptr(), cap)
            # match + triangulation of every match: one call (one launch below 16 pairs; the same outputs as the two calls, tests/test_gpu_match_tri.py)
            api.hamming_match_triangulate_batch(o["desc"].data_ptr(), o["cnt"].data_ptr(), o["desc"].data_ptr() + P * cap * 32, o["cnt"].data_ptr() + 4 * P,
                                                o["kps"].data_ptr(), o["kps"].data_ptr() + P * cap * 28, P, cap, Kt, K["bf"] / K["fx"],
                                                o["midx"].data_ptr(), o["mdist"].data_ptr(), o["xyz"].data_ptr(), o["ok"].data_ptr(), s_)
            if use_lcd and "lcd" not in skip:
                ln["lcd"].describe_batch(d_imgs.data_ptr(), P, H, W, W, H * W, o["descr"].data_ptr(), blur_in_place=False)
            if use_lcd and "db" not in skip:
                ln["D"].query_batch(o["descr"].data_ptr(), cur_ids[:P], P, o["best"].data_ptr(), o["max"].data_ptr(), o["dbcnt"].data_ptr())
            if use_ba and "ba" not in skip:
                api.ba_build_batch(*[t.data_ptr() for t in b_in], P, maxP, maxL, maxE, Kt, 5.991, *[t.data_ptr() for t in o["ba"]], s_)
        ln["body"] = body
        for _ in range(2):                               # eager first: lazy allocations, both FAST-statistics parities
            body()
        st.synchronize()
        ln["graphs"] = [api.StepGraph.record(s_, [], body) for _ in range(2)]     # two consecutive steps, replayed alternately
        ln["k"] = 0
        return ln

    def step_lanes():
        ln = lanes[step_no[0] % len(lanes)]; step_no[0] += 1
        ln["graphs"][ln["k"] & 1].launch(ln["stream"].cuda_stream); ln["k"] += 1

    def step_lanes_eager():                              # the same lanes without the recording: what the graphs save
        ln = lanes[step_no[0] % len(lanes)]; step_no[0] += 1
        ln["body"]()

    if use_graph:
        api.prof_enable(False)
        lanes = [build_lane() for _ in range(n_lanes)]
        step = step_lanes
        for _ in range(2 * n_lanes):
            step()
        barrier()

    # ---- pass 1: the timed region (no per-kernel events) ----
    api.prof_enable(False)
    clock_mhz = [api.shader_clock_mhz(stream)] if args.full else None      # --full: the shader clock, measured on the device: before the warm-up and the timed region, between the repeats, after them
    if not args.gap_before_timed:
        for _ in range(args.warmup):                     # the contract's W untimed warm-up steps, of the timed region's own kind; timed() opens with barrier + synchronize
            step()
    dt = timed(args.steps, lead=0)
    host_launch_ms = host_ms[0]
    per_rank_ms = [v / args.steps * 1e3 for v in rank_dts] if world > 1 else None            # of THIS region (the repeats below overwrite rank_dts)
    per_rank_own_ms = [v / args.steps * 1e3 for v in rank_own] if world > 1 else None
    # `value` / `ms_per_step` = THIS first region (the contract).  Two more identical regions follow at once (round 6): a box-to-box or run-to-run
    # difference of a few per cent cannot be told from a regression with one 1.3 s sample and no clock reading
    repeats_ms = [dt / args.steps * 1e3]
    for _ in range(0 if args.no_repeats else 2):
        clock_mhz.append(api.shader_clock_mhz(stream))
        repeats_ms.append(timed(args.steps, lead=0) / args.steps * 1e3)
    if clock_mhz is not None:
        clock_mhz.append(api.shader_clock_mhz(stream))
    if args.dump_outputs and rank == 0:
        # what the last timed step computed (the repeat regions run the same steps on the same inputs): the per-frame outputs of a fixed sample of frames
        fr = sample_frames(P)
        d_fr = torch.from_numpy(fr).to(dev)
        d_im = torch.cat([d_fr, d_fr + P])                    # their left, then their right images
        if use_graph:
            lo = lanes[(step_no[0] - 1) % len(lanes)]["o"]
            o_kps, o_desc, o_cnt, o_midx, o_mdist, o_xyz, o_ok = (lo[k] for k in ("kps", "desc", "cnt", "midx", "mdist", "xyz", "ok"))
            o_lcd = (lo["descr"], lo["best"], lo["max"], lo["dbcnt"]) if use_lcd else None
            o_ba = lo["ba"] if use_ba else None
        else:
            p_last = (step_no[0] - 1) % NB
            o_kps, o_desc, o_cnt = d_kps_b[p_last], d_desc_b[p_last], d_cnt_b[p_last]
            o_midx, o_mdist, o_xyz, o_ok = d_midx, d_mdist, d_xyz, d_ok
            o_lcd = (d_descr, d_best, d_max, d_dbcnt) if use_lcd else None
            o_ba = b_out if use_ba else None
        host = lambda t: t.cpu().numpy()
        n_fr = len(fr)
        write_outputs(args.dump_outputs, P, cap,
                      kps=host(o_kps.view(2 * P, cap * 28)[d_im]).view(api.KP_DTYPE).reshape(2, n_fr, cap).transpose(1, 0, 2),
                      desc=host(o_desc.view(2 * P, cap, 32)[d_im]).reshape(2, n_fr, cap, 32).transpose(1, 0, 2, 3),
                      cnt=host(o_cnt[d_im]).reshape(2, n_fr).T,
                      midx=host(o_midx.view(P, cap)[d_fr]), mdist=host(o_mdist.view(P, cap)[d_fr]),
                      xyz=host(o_xyz.view(P, cap, 3)[d_fr]), ok=host(o_ok.view(P, cap)[d_fr]),
                      lcd=None if o_lcd is None else [host(t) for t in o_lcd],
                      ba=None if o_ba is None else [host(t[d_fr]) for t in o_ba])
    if args.block_trace:                # profiling builds only: which kernel's blocks sit on which CU of XCD 0 at what time (tools/block_trace_report.py)
        import ctypes
        fn = getattr(api.lib(), "myslam_debug_block_trace")        # AttributeError = this library was not built with -DMYSLAM_BLOCK_TRACE
        fn.restype = ctypes.c_int; fn.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
        n_cap = 1 << 21
        d_bt = torch.zeros(4 * n_cap, dtype=torch.int64, device=dev)
        barrier()
        assert fn(d_bt.data_ptr(), n_cap, None) == 0
        t_bt = time.perf_counter()
        for _ in range(4):
            step()
        barrier()
        t_bt = time.perf_counter() - t_bt
        n_bt = ctypes.c_uint(0)
        assert fn(None, 0, ctypes.byref(n_bt)) == 0
        np.save(args.block_trace, d_bt[:4 * min(n_cap, n_bt.value)].cpu().numpy().view(np.uint64).reshape(-1, 4))
        print(f"block trace: {n_bt.value} records, 4 steps in {t_bt * 1e3:.2f} ms", file=sys.stderr)
        del d_bt
    # ---- multi-rank runs: the loop-database exchange timed stage by stage on an otherwise idle chip (bench/passes_multirank.py) ----
    collective = None
    if world > 1 and use_lcd and args.full:
        collective = db_exchange(api, D, world, via_cpu, dev, side_stream, d_allq, d_descr, d_cand, d_best, d_max, d_dbcnt, cur_ids, NQ, P, n_db_local)
        barrier()
    frame_latency = None
    if use_graph and args.frame_latency:
        # every step timed on ITS lane (event pair around the replay) while all lanes are busy, then one lane alone: what a camera sees
        n_probe = min(args.steps, 64 * len(lanes))
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_probe)]
        barrier()
        for a_, b_ in evs:
            ln = lanes[step_no[0] % len(lanes)]
            a_.record(ln["stream"]); step(); b_.record(ln["stream"])
        barrier()
        loaded = sorted(a_.elapsed_time(b_) for a_, b_ in evs)
        ln = lanes[0]; alone = []
        for _ in range(32):
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record(ln["stream"]); ln["graphs"][ln["k"] & 1].launch(ln["stream"].cuda_stream); ln["k"] += 1; b_.record(ln["stream"])
            ln["stream"].synchronize(); alone.append(a_.elapsed_time(b_))
        frame_latency = {"loaded_median_ms": loaded[len(loaded) // 2], "loaded_p90_ms": loaded[int(0.9 * (len(loaded) - 1))],
                         "one_lane_alone_ms": float(np.median(alone)), "steps_probed": n_probe}
    if not use_graph:
        step = step_eager

    # ---- pass 2: the same steps with a HIP event pair around every launch, on the launch's own stream ----
    prof, dt_prof = {}, None
    step_timed = step
    step = step_eager                  # every pass below launches eagerly: the profiling events, the solve cadence and the streamed input change per step
    if not args.no_extra_passes:
        for _ in range(3):                  # the pass's lead steps, BEFORE the per-launch events are switched on: the roofline objects divide event times and launch counts by args.steps
            step()
        api.prof_reset(); api.prof_enable(True)
        dt_prof = timed(args.steps, lead=0)
        api.prof_enable(False)
        prof = api.prof_read()

    # ---- pass 3: configs[3] at the reference's cadence: the solve runs per KEY-FRAME, about 1 frame in 6 ----
    cadence = None
    if use_ba and not use_solve and not args.no_extra_passes:
        solve_windows[0] = (P + 5) // 6
        api.ba_set_option(api.BA_OPT_LANDMARKS_IN_HBM, 1 if args.solve_lm_hbm else 0)
        step(); barrier()
        dt_c = timed(args.steps)
        solve_windows[0] = 0
        barrier(); api.ba_set_option(api.BA_OPT_LANDMARKS_IN_HBM, 0)
        assert int(s_st.abs().sum()) == 0
        cadence = {"value": world * P * args.steps / dt_c, "unit": "stereo frames/s", "ms_per_step": dt_c / args.steps * 1e3,
                   "solved_windows_per_step": (P + 5) // 6, "landmark_state": "hbm scratch" if args.solve_lm_hbm else "lds",
                   "note": "as the timed region, plus Backend::OptimizeActiveMap's solve stage (rounds of Levenberg-Marquardt optimize(10), Schur + "
                           "Cholesky, outlier flags) on every 6th frame's window — the reference solves per key-frame, about 1 frame in 6"}

    # ---- pass 4: streamed input — every step's images cross PCIe (app/run_kitti_stereo.cpp:61-90 reads two images per step) ----
    streamed = None
    if args.stream_input > 0 and not args.no_extra_passes:
        NBAT = args.stream_input if world == 1 else min(args.stream_input, 2)      # N ranks render on one host: two batches per rank there
        t_gen = time.perf_counter()
        h_bat = []
        for j in range(NBAT):           # consecutive frames of the same synthetic stream: batch j = frames j*P .. (j+1)*P - 1
            f = frames if j == 0 else synth.stereo_batch(P, stream_id=rank, t0=j * P, n_rect=args.scene_rects)
            h_bat.append(torch.from_numpy(np.concatenate([f[:, 0], f[:, 1]], axis=0)).pin_memory())
        t_gen = time.perf_counter() - t_gen
        NBUF = 3        # device input buffers: the copy of step k + 1 only needs step k - 2 to have finished
        d_in = [torch.empty_like(d_imgs) for _ in range(NBUF)]
        sC = torch.cuda.Stream()
        readers = [main_stream] + orb_streams + ([side_stream] if side_stream is not main_stream else [])
        ev_ready = [torch.cuda.Event() for _ in range(NBUF)]
        ev_ready2 = [torch.cuda.Event() for _ in range(NBUF)]
        sCs = [sC] + [torch.cuda.Stream() for _ in range(max(0, args.stream_split - 1))]
        ev_piece = [[torch.cuda.Event(), torch.cuda.Event()] for _ in range(NBUF)]
        ev_read = [[torch.cuda.Event() for _ in readers] for _ in range(NBUF)]
        bytes_step = h_bat[0].numel()
        k_stream = [0]
        copy_ev = []

        def step_streamed():
            k = k_stream[0]; k_stream[0] += 1
            b = k % NBUF
            for e in ev_read[b]:
                sC.wait_event(e)                    # the readers of step k - NBUF (same buffer) have finished: level 0 is read in place
            ec = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ec[0].record(sC)
            if args.stream_split and args.pipeline and S == 2:
                # the left images (extractor handle A, DeepLCD) and the right images (handle B) arrive as separate copies with an event each —
                # handle A starts when ITS half is there — on `stream_split` copy streams (1: both on one; 2: one each; 4: two each):
                # concurrent copies use more of the link (one stream sustains 51 GB/s, two 53)
                hb = h_bat[k % NBAT]
                nC = len(sCs)
                per = max(1, nC // 2)                       # copy streams per half
                for half in range(2):
                    lo, hi = half * P, (half + 1) * P
                    cs = [sCs[(half * per + j) % nC] for j in range(per)]
                    for j, c in enumerate(cs):
                        if c is not sC:
                            for e in ev_read[b]:
                                c.wait_event(e)
                        a0, a1 = lo + (hi - lo) * j // per, lo + (hi - lo) * (j + 1) // per
                        with torch.cuda.stream(c):
                            d_in[b][a0:a1].copy_(hb[a0:a1], non_blocking=True)
                    evh = ev_ready[b] if half == 0 else ev_ready2[b]
                    for c in cs[1:]:                        # the half is ready when all of its pieces are
                        ev_piece[b][half].record(c); cs[0].wait_event(ev_piece[b][half])
                    evh.record(cs[0])
                sC.wait_event(ev_ready2[b])
                ec[1].record(sC); copy_ev.append(ec)
                for st in readers:
                    st.wait_event(ev_ready2[b] if st is orb_streams[0] else ev_ready[b])
            else:
                with torch.cuda.stream(sC):
                    d_in[b].copy_(h_bat[k % NBAT], non_blocking=True)
                ec[1].record(sC); copy_ev.append(ec)
                ev_ready[b].record(sC)
                for st in readers:
                    st.wait_event(ev_ready[b])
            cur["imgs"] = d_in[b]
            step()
            for e, st in zip(ev_read[b], readers):
                e.record(st)

        for _ in range(NBUF):
            step_streamed()
        barrier()
        def signature():            # the valid descriptors of the step's first image (slots past the count hold stale bytes)
            p = (step_no[0] - 1) % NB if args.pipeline else 0
            n0 = int(d_cnt_b[p][0].item())
            return d_desc_b[p][:32 * n0].clone()
        sig_first = signature()         # of the last warm-up step
        barrier()
        copy_ev.clear()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step_streamed()
        barrier()
        dt_s = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt_s], dtype=torch.float64, device="cpu" if via_cpu else dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_s = float(t.item())
        cur["imgs"] = d_imgs
        assert all(int(t.abs().sum()) == 0 for t in d_stat_b), "ORB capacity overflow (streamed pass)"
        sig_last = signature()
        same_batch = (args.steps % NBAT) == 0          # the last timed step and the last warm-up step saw the same host batch
        assert NBAT == 1 or (sig_first.shape == sig_last.shape and torch.equal(sig_first, sig_last)) == same_batch, "streamed pass: the steps did not see the batches they were sent"
        del d_in, sig_first
        streamed = {"value": world * P * args.steps / dt_s, "unit": "stereo frames/s", "ms_per_step": dt_s / args.steps * 1e3,
                    "h2d_GBps": bytes_step * args.steps / dt_s / 1e9, "h2d_bytes_per_step": bytes_step, "distinct_batches": NBAT,
                    "host_render_s": t_gen, "h2d_copy_ms_avg": float(np.mean([a.elapsed_time(b) for a, b in copy_ev])),
                    "note": "every step extracts images that crossed PCIe for that step: consecutive frames of the synthetic stream in pinned host "
                            "memory, the left and the right images as two concurrent host->device copies per step (two copy streams), three device input buffers (a buffer is overwritten only after "
                            "every reader of the step that used it has finished — level 0 is read in place)"}

    # ---- pass 5: configs[3] read strictly — every frame is a key-frame, the solve runs on every frame's window ----
    every = None
    if use_ba and not use_solve and not args.no_extra_passes:
        solve_windows[0] = P
        step(); barrier()
        n_e = max(5, args.steps // 2)
        dt_e = timed(n_e)
        solve_windows[0] = 0
        assert int(s_st.abs().sum()) == 0
        every = {"value": world * P * n_e / dt_e, "unit": "stereo frames/s", "ms_per_step": dt_e / n_e * 1e3, "steps": n_e,
                 "note": "as the timed region, plus the OptimizeActiveMap solve stage on EVERY frame's window (configs[3] read as 'every frame is a "
                         "key-frame'; = --workload full_solve)"}

    # ---- pass 5b: the same step on a KITTI-LIKE scene.  The headline stream is deliberately hard on FAST (6 000 rectangles: 30 % of all
    # pixels are FAST-7 corners, 76 % of the pixel pairs survive the compass pre-test); street scenes are sparse (a few % corners, ~14 % of
    # the pairs survive), which is what 300 rectangles give — there FAST takes its two-phase path (pre-test, compaction, scoring of the
    # survivors only).  Reported beside `value`, never instead of it ----
    sparse = None
    if not args.no_extra_passes and world == 1 and args.scene_rects > 1000 and args.pipeline:
        fr2 = synth.stereo_batch(P, stream_id=rank, n_rect=300)
        d_sparse = torch.from_numpy(np.concatenate([fr2[:, 0], fr2[:, 1]], axis=0)).to(dev)
        keep_imgs = cur["imgs"]
        cur["imgs"] = d_sparse
        for _ in range(4):                  # the per-level path statistics of both handles settle on the new scene
            step()
        barrier()
        dt_sp = timed(args.steps)
        kp_sp = float(torch.stack([c.float().mean() for c in d_cnt_b]).mean().item())
        assert all(int(t.abs().sum()) == 0 for t in d_stat_b)
        sparse = {"value": world * P * args.steps / dt_sp, "unit": "stereo frames/s", "ms_per_step": dt_sp / args.steps * 1e3, "scene_rects": 300,
                  "keypoints_per_image": kp_sp,
                  "note": "the timed region on a sparse, street-like scene (300 rectangles instead of 6 000): FAST chooses its two-phase path per level "
                          "from the previous launch's statistics; same kernels, same outputs (tests/test_gpu_fallbacks.py)"}
        cur["imgs"] = keep_imgs
        for _ in range(4):
            step()
        barrier()
        del d_sparse

    # ---- pass 6: the extractor ALONE on an otherwise idle chip (three calls of one handle, event pair around every launch): what a launch
    # of each ORB kernel takes when nothing shares its CUs — under the pipeline a launch is resident for longer BY DESIGN (blocks of the
    # other streams move in beside FAST's), so the per-launch durations of pass 2 price the schedule, these price the kernel ----
    alone = {}
    if not args.no_extra_passes:
        barrier()
        api.prof_reset(); api.prof_enable(True)
        n_alone = 2 * P // S
        for _ in range(3):
            ext.detect_and_compute_batch(cur["imgs"].data_ptr(), n_alone, H, W, W, H * W, d_kps_b[0].data_ptr(), d_desc_b[0].data_ptr(),
                                         d_cnt_b[0].data_ptr(), d_stat_b[0].data_ptr(), cap)
        torch.cuda.synchronize()
        api.prof_enable(False)
        alone = {k: v for k, v in api.prof_read().items() if v[1] > 0}

    emulated = None
    if emu and use_lcd:
        # the same scan and merge on an otherwise idle chip (HIP events on the side stream), beside what they took inside the pipeline (profiled pass)
        barrier()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        acc = np.zeros(2)
        with torch.cuda.stream(side_stream):
            for it in range(-2, 10):
                evs[0].record(side_stream)
                D.query_batch_sharded(d_allq.data_ptr(), cur_ids, NQ, d_gath.data_ptr()); evs[1].record(side_stream)
                api.lcd_merge_candidates_device(d_gath.data_ptr(), emu, NQ, d_best.data_ptr(), d_max.data_ptr(), d_dbcnt.data_ptr(), stream2); evs[2].record(side_stream)
                side_stream.synchronize()
                if it >= 0:
                    acc += np.array([evs[0].elapsed_time(evs[1]), evs[1].elapsed_time(evs[2])])
        scan_in = prof.get("lcddb_scan")
        emulated = {"world": emu, "shard_rows": int(n_db_local), "queries_scanned_per_step": int(NQ), "candidate_sets_merged": emu,
                    "shard_scan_ms_per_step": None if not scan_in or not scan_in[1] else scan_in[0] / args.steps,
                    "shard_scan_alone_ms": float(acc[0] / 10), "merge_alone_ms": float(acc[1] / 10),
                    "ms_per_step": dt / args.steps * 1e3, "per_rank_frames_per_s": P * args.steps / dt,
                    "not_included": "the two all-gathers of a real N-GPU job (queries: N x P x 4 256 B, candidates: N x N P x 16 B); DESIGN.md section 4 keeps those modelled",
                    "note": "one process, one GPU, no collective: this rank's per-step compute as rank 0 of an N-rank job — N P queries against its 6 250-row shard "
                            "(event-timed inside the pipelined schedule by the profiled pass: shard_scan_ms_per_step) and the merge of N candidate sets"}
    # (this pass comes last of the timed ones: the lanes bring their own streams, and on this runtime streams beyond GPU_MAX_HW_QUEUES share
    # hardware queues — created before the streamed-input pass they cost it a third of its rate, 38.5 k instead of 57 k frames/s)
    # the other launch mode over the same steps (eager when the timed region replayed graphs, graphs when it launched eagerly)
    other_mode = None
    lanes_eager = None
    if can_graph and not args.no_extra_passes:
        if not use_graph:
            api.prof_enable(False)
            lanes = [build_lane() for _ in range(n_lanes)]
        fn_o = step_eager if use_graph else step_lanes
        for _ in range(2 * n_lanes):
            fn_o()
        barrier()
        dt_o = timed(args.steps, fn_o)
        other_mode = {"mode": "eager launches, two extractor handles + match + side chain on four streams, consecutive steps overlap" if use_graph else
                              f"HIP graph replay on {n_lanes} single-stream lanes",
                      "value": world * P * args.steps / dt_o, "unit": "stereo frames/s", "ms_per_step": dt_o / args.steps * 1e3,
                      "host_launch_ms_per_step": host_ms[0], "graph_nodes": lanes[0]["graphs"][0].node_count()}
        for _ in range(2 * n_lanes):
            step_lanes_eager()
        barrier()
        dt_l = timed(args.steps, step_lanes_eager)
        lanes_eager = {"mode": f"the same {n_lanes} lanes launched eagerly (no recording)", "value": world * P * args.steps / dt_l,
                       "ms_per_step": dt_l / args.steps * 1e3, "host_launch_ms_per_step": host_ms[0]}
    if args.verify and args.pipeline:
        # the overlapped schedule must not change a single output: one plain step (handles un-gated, joined) against the last pipelined one
        outs = lambda p: [d_kps_b[p], d_desc_b[p], d_cnt_b[p], d_stat_b[p], d_midx, d_mdist, d_xyz, d_ok] + \
            ([d_descr, d_best, d_max, d_dbcnt] if use_lcd else []) + (list(b_out) if use_ba else [])
        torch.cuda.synchronize()
        for p in range(NB):             # both sides start from cleared buffers: slots behind an image's count keep whatever an earlier pass
            for t in outs(p):           # (the streamed one extracts other frames) left there, and whole buffers are compared
                t.zero_()
        step(); torch.cuda.synchronize()
        p_last = (step_no[0] - 1) % NB
        ref = [t.clone() for t in outs(p_last)]
        for e in exts:
            e.set_fast_event(0); e.set_fast_gate(0)
        for t in outs(0):
            t.zero_()
        step_joined()
        torch.cuda.synchronize()
        for i, (a, r) in enumerate(zip(outs(0), ref)):            # every output, the f64 BA blocks included, is bit-reproducible
            assert torch.equal(a.view(torch.uint8), r.view(torch.uint8)), f"pipeline output {i} differs from the joined step"
        for i, e in enumerate(exts):
            e.set_fast_event(ev_fast[i].cuda_event)
            if args.pipeline == 1:
                e.set_fast_gate(ev_fast[(i - 1) % S].cuda_event)
    if args.verify and lanes:           # a recorded step on a lane against the joined eager step: every output bit for bit
        torch.cuda.synchronize()
        step_joined(); torch.cuda.synchronize()
        refs = {"kps": d_kps, "desc": d_desc, "cnt": d_cnt, "midx": d_midx, "mdist": d_mdist, "xyz": d_xyz, "ok": d_ok}
        if use_lcd:
            refs.update({"descr": d_descr, "best": d_best, "max": d_max, "dbcnt": d_dbcnt})
        n0 = [int(v) for v in d_cnt.cpu()]
        for ln in lanes[:2]:
            for rep in range(2):
                ln["graphs"][rep].launch(ln["stream"].cuda_stream); ln["stream"].synchronize()
                lo = ln["o"]
                assert torch.equal(lo["cnt"], d_cnt) and int(lo["stat"].abs().sum()) == 0
                kl = lo["kps"].view(2 * P, cap * 28); kr = d_kps.view(2 * P, cap * 28); dl = lo["desc"].view(2 * P, cap * 32); dr = d_desc.view(2 * P, cap * 32)
                for b_ in range(2 * P):             # slots behind an image's count are never written
                    assert torch.equal(kl[b_, :28 * n0[b_]], kr[b_, :28 * n0[b_]]) and torch.equal(dl[b_, :32 * n0[b_]], dr[b_, :32 * n0[b_]]), f"lane key-points / descriptors, image {b_}"
                for b_ in range(P):
                    sl = slice(b_ * cap, b_ * cap + n0[b_])
                    assert torch.equal(lo["midx"][sl], d_midx[sl]) and torch.equal(lo["mdist"][sl], d_mdist[sl]) and torch.equal(lo["ok"][sl], d_ok[sl])
                    assert torch.equal(lo["xyz"].view(-1, 3)[sl].view(torch.uint8), d_xyz.view(-1, 3)[sl].view(torch.uint8))
                for k_ in ("descr", "best", "max", "dbcnt"):
                    if k_ in lo:
                        assert torch.equal(lo[k_].view(torch.uint8), refs[k_].view(torch.uint8)), f"lane output {k_}"
                if use_ba:
                    for a_, r_ in zip(lo["ba"], b_out):
                        assert torch.equal(a_.view(torch.uint8), r_.view(torch.uint8)), "lane BA blocks"

    # ---- parity sample: K frames of one more step of the timed workload against the oracle (untimed; beside cpu_baseline) ----
    parity = None
    if rank == 0 and args.parity_frames > 0 and world == 1:
        barrier()
        step_timed(); barrier()                         # the launch mode of the timed region (a graph replay on a lane for small batches)
        host = lambda t: t.cpu().numpy()
        if use_graph:
            lo = lanes[(step_no[0] - 1) % len(lanes)]["o"]
            bufs = {k: (host(v) if k != "ba" else [host(t) for t in v]) for k, v in lo.items() if k != "stat"}
        else:
            p_last = (step_no[0] - 1) % NB
            bufs = {"kps": host(d_kps_b[p_last]), "desc": host(d_desc_b[p_last]), "cnt": host(d_cnt_b[p_last]), "midx": host(d_midx), "mdist": host(d_mdist),
                    "xyz": host(d_xyz), "ok": host(d_ok)}
            if use_lcd:
                bufs.update({"descr": host(d_descr), "best": host(d_best), "max": host(d_max), "dbcnt": host(d_dbcnt)})
            if use_ba:
                bufs["ba"] = [host(t) for t in b_out]
        kf = min(args.parity_frames, P)
        sample = sorted({int(round(j * (P - 1) / max(1, kf - 1))) for j in range(kf)})
        parity = parity_sample(api, synth, frames, sample, cap, Kt, K, bufs, db_np, ids if use_lcd else None, int(cur_ids[0]) if use_lcd else 0,
                               ba_w, synth.calc_weights())

    solve_ms = None; solve_roof = None
    if use_ba and not use_solve and not args.no_extra_passes:        # the solve of ALL P windows, timed on its own (not part of `value`)
        with torch.cuda.stream(side_stream):
            solve(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(5):
                solve()
            torch.cuda.synchronize()
        solve_ms = (time.perf_counter() - t1) / 5 * 1e3
        assert int(s_st.abs().sum()) == 0
        solve_roof = ba_solve_roofline(s_rd.cpu().numpy(), ba_w[6], P, solve_ms)

    # ---- pass: the database GROWS inside the step (round 6).  The reference appends every key-frame (AddToDatabase) after its DetectLoop; the timed region scans a
    # database that was loaded once.  Here every step appends its key-frames (1 frame in 6) behind its scan, asynchronously on the side stream (myslam_lcddb_append_batch_async),
    # and the next step scans them too.  After everything that reads the original database (parity sample above) ----
    db_grow = None
    if use_lcd and world == 1 and not emu and not args.no_extra_passes and args.pipeline:
        nkf = (P + 5) // 6
        n0 = len(D)
        D.reserve(n0 + (args.steps + 4) * nkf)             # growth moves the matrix (a synchronising operation): room for the whole pass up front
        keep_cur = cur_ids.copy()
        grow[0], grow[1], grow[2] = True, int(ids[-1]) + 1, []
        grow[3] = torch.empty(args.steps + 4, nkf, 1064, device=dev)       # the key-frame rows of every step of the pass (kept for the check below)
        step(); step(); barrier()
        dt_g = timed(args.steps, lead=0)                   # (the two steps above are its lead; every step appends, and the row count below is checked)
        grow[0] = False
        n1 = len(D)
        dt_big = timed(args.steps)                          # the same steps against the database as it has become, nothing appended: what the larger scan alone costs
        # check: the key-frames of the LAST step are in the database under their ids — queried with their own descriptors they come back with score 1
        last = grow[2][-1]
        qb = torch.zeros(nkf, dtype=torch.int64, device=dev); qm = torch.zeros(nkf, device=dev); qc = torch.zeros(nkf, dtype=torch.int32, device=dev)
        with torch.cuda.stream(side_stream):
            D.query_batch(last.data_ptr(), np.full(nkf, grow[1] + 1000, np.uint64), nkf, qb.data_ptr(), qm.data_ptr(), qc.data_ptr())
        torch.cuda.synchronize()
        # (every step of the bench extracts the same 512 pairs, so every step appends the same 86 descriptors: the strict-'>' scan returns the FIRST copy of each)
        first_ids = np.arange(int(ids[-1]) + 1, int(ids[-1]) + 1 + nkf, dtype=np.uint64)
        found = int((torch.from_numpy(first_ids.view(np.int64)).to(dev) == qb).sum()); smin = float(qm.min())
        copies = int(qc.min())                            # every query sees all copies of its row above the 0.92 threshold: at least one per step
        db_grow = {"value": world * P * args.steps / dt_g, "unit": "stereo frames/s", "ms_per_step": dt_g / args.steps * 1e3, "key_frames_appended_per_step": nkf,
                   "rows_before": n0, "rows_after": n1, "ms_per_step_at_rows_after_without_appends": dt_big / args.steps * 1e3, "last_step_key_frames_found_at_their_first_copy": found, "of": nkf, "their_min_score": smin, "min_rows_above_threshold": copies,
                   "ok": bool(n1 == n0 + (args.steps + 2) * nkf and found == nkf and smin > 0.9999 and copies >= args.steps + 2),
                   "note": "as the timed region, plus LoopClosing::AddToDatabase inside the step: every step appends its key-frames (1 frame in 6) behind its scan with "
                           "myslam_lcddb_append_batch_async on the side stream (no host wait) and the following steps scan them; rows reserved up front"}
        cur_ids[:] = keep_cur; grow[2] = []; grow[3] = None
        assert db_grow["ok"], db_grow
    if rank == 0 and world == 1 and args.stream_mode and not args.no_extra_passes and args.workload in ("full", "orb_match_lcd") and args.stream_mode_late:
        barrier()
        stream_mode = stream_mode_sweep(args)       # (A/B only: the children run beside this process's idle GPU context)
    if rank == 0:
        ms_step = dt / args.steps * 1e3
        value = world * P * args.steps / dt
        roof, roof_valu, mf, busy, peaks = None, None, None, {}, None
        if args.full:
            roof, roof_valu, mf, busy, peaks = rooflines(prof, alone, args.steps, P, lcd.conv2_products() if use_lcd else 3, build_id=api.build_id())
        n_internal = S if args.orb_internal_stream else 0        # every extractor handle runs its Gaussian pyramid on an internal stream
        out = {
            "metric": "stereo frames/sec (ORB+match+LCD+BA-build) @1241x376",
            "value": value, "unit": "stereo frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "repeats_ms_per_step": repeats_ms,          # [the timed region behind `value`, two more identical regions run straight after it]
            "clock_mhz": clock_mhz,                     # shader clock measured on the device before / between / after those regions (one idle-chip wave each)
            "library": api.version(),
            "dtype": "u8/int32 (ORB, Hamming), f32 via f16x3 / bf16x6 split products on the matrix cores with f32 accumulate (CALC conv1 / conv2, DB scan), "
                     "f64 (triangulation, BA)", "data": "synthetic",
            "config": {"workload": {"full": "configs[3]: ORB extract L+R (2000 feats) + L/R Hamming match + triangulation + DeepLCD descriptor + "
                                            f"{n_db_local * world}-KF cosine DB scan + local-BA (10 KF x 300 MP, one distinct window per frame) block build",
                                    "full_solve": "configs[3] incl. solve on EVERY frame: as 'full' + the Backend::OptimizeActiveMap solve stage (rounds of "
                                                  "Levenberg-Marquardt optimize(10) with Schur + Cholesky, outlier flags) of the 10 KF x 300 MP window",
                                    "orb_match": "configs[1]: ORB extract L+R (2000 feats) + L/R Hamming match + triangulation",
                                    "orb_match_lcd": f"configs[2]: configs[1] + DeepLCD descriptor + {n_db_local * world}-KF cosine DB scan"}[args.workload],
                       "pairs_per_step_per_gpu": P, "image": "1241x376 u8", "scene_rects": args.scene_rects, "keypoints_per_image": n_kp,
                       "hip_streams": {"caller": len({stream, stream2} | {s.cuda_stream for s in orb_streams}) + (1 if args.pipeline else 0),
                                       "extractor_internal": n_internal},
                       "hip_hw_queues": int(HW_QUEUES), "hip_dev_kernarg": DEV_KERNARG, "orb_extractor_handles": S, "pipelined_steps": bool(args.pipeline),
                       "input_level0": "read in place (resident input images; the last image of each extractor call is copied)" if not args.orb_copy_input
                                       else "copied into the pyramid block",
                       "parallelism": f"frame-sharded x{world}" + (", id-range sharded DB + all-gather of 16-byte candidate records" if world > 1 else "")},
            "rccl_ranks": rccl_ranks if not via_cpu else None, "collective_backend": (args.backend if world > 1 else None),
            "collective_ranks": rccl_ranks,
            "per_rank_ms_per_step": per_rank_ms, "per_rank_own_device_done_ms_per_step": per_rank_own_ms,
            "collective_ms_per_step": None if collective is None else collective["collective_ms_per_step"],
            "shard_scan_ms_per_step": None if collective is None else collective["shard_scan_ms_per_step"],
            "db_exchange": collective, "emulated_world": emulated, "db_grow": db_grow,
            "roofline": roof, "roofline_valu": roof_valu, "roofline_mfma": mf,
            "profiled_pass": None if dt_prof is None else {"ms_per_step": dt_prof / args.steps * 1e3,
                                                           "kernel_ms_per_step": {SYMBOL.get(k, k): v[0] / args.steps for k, v in busy.items()}},
            "extractor_alone": None if not alone else {"images_per_call": 2 * P // S, "calls": 3,
                                                       "kernel_ms_per_call": {SYMBOL.get(k, k): v[0] / 3 for k, v in alone.items()},
                                                       "note": "pass 6: one extractor handle on an otherwise idle chip; event-timed launches"},
            "streamed": None if streamed is None else dict(streamed, ratio_to_resident=streamed["value"] / value,
                                                           pcie_h2d_measured_GBps=(peaks or {}).get("h2d_GBps"),
                                                           pcie_bound_frames_per_s=None if not (peaks or {}).get("h2d_GBps") else
                                                           world * (peaks["h2d_GBps"] * 1e9) / (2 * H * W)),
            "full_solve_cadence6": cadence, "full_solve_every_frame": every, "kitti_like_scene": sparse,
            "launch_mode": f"HIP graph replay on {n_lanes} single-stream lanes (step k on lane k mod {n_lanes})" if use_graph else
                           "eager launches (two extractor handles + match + side chain on four streams, consecutive steps overlap)",
            "host_launch_ms_per_step": host_launch_ms,      # CPU time of enqueuing one step of the timed region
            "graph_nodes": lanes[0]["graphs"][0].node_count() if (use_graph and lanes) else None,
            ("step_eager" if use_graph else "step_graph"): other_mode, "step_lanes_eager": lanes_eager,
            "ba_solve_all_windows_ms": solve_ms,     # OptimizeActiveMap solve stage for all P windows, outside the timed region
            "roofline_ba_optimize": solve_roof,
            "parity_sample": parity,
            "stream_mode": stream_mode, "frame_latency": frame_latency,
        }
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(synth, args.workload, args.cpu_pairs, db_np if db_np is not None else synth.lcd_database(16), frames,
                                               ba_w if ba_w is not None else synth.ba_windows(2)[0])
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out))
        if parity is not None and not parity["ok"]:
            print("parity_sample FAILED: " + "; ".join(parity["mismatches"][:8]), file=sys.stderr)
            sys.exit(3)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
