"""bench.py prints exactly one JSON line with the driver's contract fields, the roofline and the CPU-baseline objects (small run)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [["--cpu-pairs", "2", "--verify"], ["--no-cpu-baseline", "--workload", "orb_match", "--streams", "1"]])
def test_bench_json_contract(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "16", "--full"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "profiled_pass", "rccl_ranks"):
        assert k in d, k
    assert d["roofline"]["kernel"].startswith("k_")               # the profiled kernel by its symbol
    assert d["config"]["hip_streams"]["caller"] >= 1
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"] and d["value"] > 0
    assert abs(d["value"] - 16 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    # round 6: the line carries its own spread — the timed region behind `value` plus two identical regions straight after it, the shader clock measured
    # on the device around them, and the library's build digest; the committed counter file says which build it was taken on and whether that is this one
    rp = d["repeats_ms_per_step"]
    assert len(rp) == 3 and rp[0] == d["ms_per_step"] and all(v > 0 for v in rp)
    assert len(d["clock_mhz"]) == 4 and all(300.0 < c < 3000.0 for c in d["clock_mhz"]), d["clock_mhz"]
    assert d["library"].startswith("myslam_hip ") and " build " in d["library"]
    if "lcd" in d["config"]["workload"].lower():
        # round 6: the database GROWS inside the step (AddToDatabase behind every step's DetectLoop, asynchronously on the side stream), checked after the pass
        g = d["db_grow"]
        assert g and g["ok"] is True and g["rows_after"] == g["rows_before"] + (d["steps"] + 2) * g["key_frames_appended_per_step"] and g["value"] > 0
    roof = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    if roof["traffic"] is not None:
        assert isinstance(roof["traffic_stale"], bool) and roof["traffic_build"]
        assert roof["traffic_stale"] == (roof["traffic_build"] != d["library"].rsplit(" ", 1)[-1])
    assert roof["bound"] in ("hbm", "mfma") and roof["peak"] > 0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    # the streamed-input pass: every step's images cross PCIe; three distinct host batches here
    st = d["streamed"]
    assert st and st["value"] > 0 and st["distinct_batches"] == 4 and st["h2d_bytes_per_step"] == 2 * 16 * 376 * 1241
    assert abs(st["h2d_GBps"] - st["h2d_bytes_per_step"] / (st["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * st["h2d_GBps"]
    # normalisations: every frac is achieved / peak, and the matrix-core one is priced against the bf16 dense peak (cannot exceed 1)
    if d.get("roofline_mfma"):
        mf = d["roofline_mfma"]
        assert mf["peak"] == 2500.0 and abs(mf["frac"] - mf["achieved"] / mf["peak"]) < 1e-9 and mf["frac"] < 1.0
    if d.get("roofline_valu"):
        rv = d["roofline_valu"]
        assert abs(rv["frac"] - rv["achieved"] / rv["peak"]) < 1e-9 and 30.0 < rv["peak"] < 45.0
    # the dominant kernel's launch on an idle chip (pass 6) beside its launch under the pipeline
    if d["roofline"].get("alone"):
        al = d["roofline"]["alone"]
        # (no ordering asserted between the two durations: at this test's 16 pairs per step a launch is too short for the pipeline to stretch it)
        assert al["avg_launch_ms"] > 0 and abs(al["frac"] - al["achieved"] / roof["peak"]) < 1e-9
        assert d["extractor_alone"]["kernel_ms_per_call"]["k_fast_strip"] > 0
    km = d["profiled_pass"]["kernel_ms_per_step"]
    if "lcd" in d["config"]["workload"].lower():
        assert "k_conv3_norm" in km and "k_pool_lrn128_2x2" in km and "k_conv2_f16x3" in km
    # the oracle parity sample of the timed workload (frames of one more step of the same step function, pulled after the timed region)
    ps = d["parity_sample"]
    assert ps and ps["ok"] is True and ps["mismatches"] == [] and ps["frames"] == 8 and ps["pairs_per_step"] == 16
    assert ps["orb"] == "bit-exact" and ps["match"] == "bit-exact" and ps["keypoints_compared"] > 8 * 2 * 1500 and ps["triangulation_max_rel"] <= 1e-9
    if "lcd" in d["config"]["workload"].lower():
        assert ps["lcd_max_abs"] < 2e-5 and ps["db_score_max_abs"] < 2e-5 and ps["ba_max_rel"] <= 1e-11
    else:
        assert ps["lcd_max_abs"] is None and ps["ba_max_rel"] is None
    # live-stream operating points (children of the run): one pair per step first, every point parity-checked against the oracle
    if "lcd" in d["config"]["workload"].lower():
        sm = d["stream_mode"]
        assert sm and sm["pairs_per_step"] == 1 and sm["lanes"] >= 8 and sm["value"] > 0 and len(sm["sweep"]) >= 3
        assert all(p.get("parity_ok") is True and p["frame_latency_ms"]["one_lane_alone_ms"] > 0 for p in sm["sweep"]), sm["sweep"]
    if "--no-cpu-baseline" in extra:
        assert d["cpu_baseline"] is None
    else:
        cb = d["cpu_baseline"]
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in cb, k
        assert cb["kind"] in ("port", "reference") and cb["value"] > 0 and cb["cores"] >= 1


def test_bench_two_ranks_on_one_gpu():
    """The N>1 path of bench.py (frame sharding, id-range sharded loop DB + all-gather, barrier, max over ranks, one JSON line from
    rank 0) launched exactly as the driver launches it, with both ranks on the only GPU of the box and gloo carrying the collectives."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs", "16",
           "--backend", "gloo", "--verify", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["cpu_baseline"] is None        # CPU baseline: rank 0 at N=1 only
    assert abs(d["value"] - 2 * 16 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]       # whole-job rate: both ranks' pairs
    assert "x2" in d["config"]["parallelism"] and d["collective_ranks"] == 2
    # the self-explaining part of a multi-rank line: every rank's own time, and the loop-database exchange stage by stage
    assert len(d["per_rank_ms_per_step"]) == 2 and max(d["per_rank_ms_per_step"]) == pytest.approx(d["ms_per_step"], rel=1e-9)
    own = d["per_rank_own_device_done_ms_per_step"]
    assert len(own) == 2 and all(0 < o <= w + 1e-9 for o, w in zip(own, d["per_rank_ms_per_step"]))
    x = d["db_exchange"]
    assert d["collective_ms_per_step"] == x["collective_ms_per_step"] > 0 and d["shard_scan_ms_per_step"] == x["shard_scan_ms_per_step"] > 0
    assert len(x["allgather_queries_ms"]) == len(x["allgather_candidates_ms"]) == len(x["shard_scan_ms"]) == 2
    assert x["allgather_queries_bytes_per_rank"] == 16 * 1064 * 4 and x["allgather_candidates_bytes_per_rank"] == 32 * 16 and x["queries_scanned_per_rank"] == 32


def test_bench_self_launch_two_ranks():
    """`python bench.py --gpus 2` without torch.distributed.run: bench.py starts its ranks itself (gloo here: both ranks share the
    box's only GPU; with the default nccl backend each rank takes its own GPU and the JSON carries rccl_ranks)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs", "16", "--backend", "gloo",
           "--no-extra-passes"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["collective_ranks"] == 2 and d["collective_backend"] == "gloo" and d["value"] > 0


def test_bench_self_launch_eight_ranks():
    """BASELINE configs[4]'s rank count on one GPU: `python bench.py --gpus 8 --backend gloo --pairs 8` — the 8-rank code path (8 id-range
    shards, check_shard_order, NQ = 8 P queries per shard scan, two all-gathers per step, the 8-way candidate merge) so that the first real
    8-GPU run cannot fail on something two ranks never exercised."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--pairs", "8", "--backend", "gloo",
           "--db", "640", "--stream-input", "2", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["collective_ranks"] == 8 and d["collective_backend"] == "gloo" and d["scaling"] == "weak"
    assert abs(d["value"] - 8 * 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]        # whole-job rate over all 8 ranks
    assert "x8" in d["config"]["parallelism"] and "5120-KF" in d["config"]["workload"]
    assert d["streamed"]["value"] > 0 and d["full_solve_cadence6"]["value"] > 0
    assert len(d["per_rank_ms_per_step"]) == 8 and len(d["db_exchange"]["shard_scan_ms"]) == 8 and d["db_exchange"]["shard_rows"] == 640


@pytest.mark.parametrize("graph", ["1", "0"])
def test_bench_plain_line_and_dumped_outputs(graph, tmp_path, synth, oracle):
    """The plain command (no --full) times its steps and prints the line, nothing measured by a pass of its own; --dump-outputs writes what the last timed
    step computed (float32 / float64, at most 64 MB), the sampled frames' key-points bit-exact with the oracle on those frames' images.  graph 1 = the
    recorded steps on lanes (the small-batch default), graph 0 = the pipelined eager schedule (the default at 512 pairs)."""
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "16", "--graph", graph,
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"].startswith("stereo frames/sec") and d["unit"] == "stereo frames/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["steps"] == 3 and d["warmup"] == 1 and abs(d["value"] - 16 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    assert d["repeats_ms_per_step"] == [d["ms_per_step"]] and d["clock_mhz"] is None
    for k in ("roofline", "profiled_pass", "full_solve_cadence6", "streamed", "parity_sample", "cpu_baseline", "stream_mode", "db_grow", "extractor_alone"):
        assert not d[k], k
    files = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert {"sample_frames", "orb_count", "orb_keypoints", "orb_descriptors", "match_index", "triangulated_xyz", "lcd_descriptor", "db_best_id", "ba_Hpp"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20
    fr = files["sample_frames"].astype(int)
    assert list(fr) == list(range(16)) and files["orb_count"].shape == (16, 2) and files["lcd_descriptor"].shape == (16, 1064)
    frames = synth.stereo_batch(16, stream_id=0, n_rect=6000)
    for side in range(2):
        kp, desc = oracle.detect_and_compute(oracle.params(2000), frames[fr[5], side])
        n = int(files["orb_count"][5, side])
        assert n == len(kp) > 1000
        got = files["orb_keypoints"][5, side]
        ref = np.stack([kp[f].astype(np.float32) for f in ("x", "y", "size", "angle", "response", "octave", "class_id")], -1)
        assert np.array_equal(got[:n], ref) and not got[n:].any()
        assert np.array_equal(files["orb_descriptors"][5, side, :n], desc.astype(np.float32))
