"""CPU checks of the parts of bench.py that need no GPU (package bench/): the command line's defaults (the driver runs `python bench.py --gpus N
--steps K --warmup W`; with no flags N = 1), the roofline objects built from event times + the committed counter / peak files, the solve's flop
model.  The GPU run of the whole line is tests/test_gpu_bench_contract.py."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_command_line_defaults(monkeypatch):
    from bench.args import parse
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = parse()
    assert a.gpus == 1 and a.steps == 200 and a.warmup == 5 and a.pairs == 512 and a.workload == "full"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "3"])
    a = parse()
    assert (a.gpus, a.steps, a.warmup) == (8, 20, 3)
    # a plain run is the timed region only; --full adds every other pass with today's defaults
    assert not a.full and a.dump_outputs == "" and a.no_extra_passes and a.no_repeats and a.no_cpu_baseline and a.parity_frames == 0 and a.stream_mode == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = parse()
    assert a.full and a.dump_outputs == "out" and not (a.no_extra_passes or a.no_repeats or a.no_cpu_baseline)
    assert a.parity_frames == 8 and a.stream_input == 4 and a.stream_mode == "1x16,1x4,2x16,4x16"


def test_roofline_objects_from_event_times():
    """rooflines(): the dominant kernel of the ORB chain is the one with the largest VALU volume in the committed counter summary (FAST), its HBM
    view = algorithmic bytes per launch / event-timed launch duration, its VALU view = counted wave-instructions x 64 / duration against the
    measured packed-16 peak; conv2 against the dense 16-bit matrix-core peak."""
    from bench.config import ALGO_BYTES, HBM_PEAK_GBS
    from bench.report import ba_solve_roofline, rooflines
    steps, P = 10, 512
    # {slot: (total ms, launches)}: two FAST launches of 512 images per step, each 3.0 ms; conv2 one launch of 3.1 ms per step
    prof = {"fast": (2 * 3.0 * steps, 2 * steps), "resize": (14 * 0.1 * steps, 14 * steps), "describe": (2 * 1.6 * steps, 2 * steps),
            "calc_conv2": (3.1 * steps, steps), "octree": (0.7 * steps, 2 * steps), "unused": (0.0, 0)}
    alone = {"fast": (3 * 1.4, 3)}
    roof, valu, mfma, busy, peaks = rooflines(prof, alone, steps, P, 3)
    assert "unused" not in busy and roof["stage"] == "fast" and roof["kernel"].startswith("k_fast_strip")
    assert roof["images_per_launch"] == 512 and roof["avg_launch_ms"] == pytest.approx(3.0)
    assert roof["achieved"] == pytest.approx(ALGO_BYTES["fast"] * 512 / 3.0e-3 / 1e9) and roof["frac"] == pytest.approx(roof["achieved"] / HBM_PEAK_GBS)
    assert roof["alone"]["avg_launch_ms"] == pytest.approx(1.4) and roof["alone"]["frac"] > roof["frac"]
    assert roof["traffic"] is not None and 0.9 < roof["traffic"] / roof["algorithmic_bytes_per_launch"] < 1.2          # counter traffic ~ algorithmic bytes
    assert valu["bound"] == "valu" and 1.3e6 < valu["valu_wave_insts_per_image"] < 1.7e6
    assert valu["achieved"] == pytest.approx(valu["valu_wave_insts_per_image"] * 512 * 64 / 3.0e-3 / 1e12) and 0.3 < valu["frac"] < 0.6 and 0.8 < valu["frac_alone"] < 1.1
    assert mfma["kernel"] == "k_conv2_f16x3" and mfma["partial_products"] == 3
    assert mfma["achieved"] == pytest.approx(3 * 2 * 176160768 * P / 3.1e-3 / 1e12) and mfma["frac"] == pytest.approx(mfma["achieved"] / 2500.0)
    assert roof["traffic_stale"] is None and roof["traffic_build"]            # no library named: staleness unknown, the counter file still names its build
    roof_s = rooflines(prof, alone, steps, P, 3, build_id="not-the-profiled-build")[0]
    assert roof_s["traffic_stale"] is True
    json.dumps([roof, valu, mfma])                                            # everything in the line is JSON
    # nothing profiled: the contract's object with nulls, no exception
    roof0, valu0, mfma0, _, _ = rooflines({}, {}, steps, P, 3)
    assert roof0["bound"] == "hbm" and roof0["achieved"] is None and valu0 is None and mfma0 is None
    # the solve's flop model: rounds EXECUTED = rounds failed + 1, at most 5
    sizes = np.tile(np.array([[10, 300, 2950]]), (4, 1))
    r = ba_solve_roofline(np.array([0, 0, 4, 9]), sizes, 4, 2.0)
    assert r["rounds_executed_mean"] == pytest.approx((1 + 1 + 5 + 5) / 4) and r["windows_per_launch"] == 4 and 0 < r["frac"] < 1


def test_committed_profiles_are_the_newest_of_their_kind():
    from bench.profiles import peaks_file, pmc_file
    pmc, path = pmc_file()
    assert pmc is not None and path.startswith(("profiles/r05_pmc_", "profiles/r06_pmc_")) and any(k.startswith("k_fast_strip<32, 4, 40") for k in pmc["kernels"])      # (the committed profiles name the instance "<32, 4, 40, 1>", from when it had a fourth template argument; new traces say "<32, 4, 40>")
    assert abs(pmc["calibration"]["fetch_scale"] - 1.93) < 0.05                # gfx950 counts 128-byte requests as 64 bytes (MI355X_MICROARCH.md)
    peaks, ppath = peaks_file()
    assert peaks and os.path.exists(os.path.join(ROOT, ppath)) and 5500 < peaks["hbm_copy_GBps"] < 8000


def test_dump_outputs_layout(tmp_path):
    """bench.py --dump-outputs: float32 / float64 arrays only, slots past an image's count zeroed (the step never writes them), the sample fixed by its seed."""
    from bench.dump import sample_frames, write
    api_dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
    P, cap = 512, 40
    fr = sample_frames(P)
    assert len(fr) == 16 and list(fr) == sorted(set(fr)) and np.array_equal(fr, sample_frames(P)) and list(sample_frames(8)) == list(range(8))
    n = len(fr)
    rng = np.random.default_rng(1)
    kps = np.zeros((n, 2, cap), api_dtype)
    for f in api_dtype.names:
        kps[f] = rng.integers(1, 100, kps.shape)
    desc = rng.integers(1, 256, (n, 2, cap, 32)).astype(np.uint8)
    cnt = rng.integers(0, cap + 1, (n, 2)).astype(np.int32)
    midx = rng.integers(1, 100, (n, cap)).astype(np.int32); xyz = rng.standard_normal((n, cap, 3)) + 5
    ok = np.ones((n, cap), np.uint8)
    lcd = (rng.random((P, 1064), dtype=np.float32), np.arange(P, dtype=np.int64), rng.random(P, dtype=np.float32), np.ones(P, np.int32))
    ba = [rng.standard_normal((n, m)) for m in (36, 9, 18, 6, 3, 1)]
    names = write(str(tmp_path), P, cap, kps, desc, cnt, midx, midx, xyz, ok, lcd=lcd, ba=ba)
    got = {m: np.load(os.path.join(tmp_path, m + ".npy")) for m in names}
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == names and all(a.dtype in (np.float32, np.float64) for a in got.values())
    k = got["orb_keypoints"]
    assert k.shape == (n, 2, cap, 7) and got["orb_descriptors"].shape == (n, 2, cap, 32) and got["triangulated_xyz"].shape == (n, cap, 3)
    for i in range(n):
        for s in range(2):
            c = cnt[i, s]
            assert np.array_equal(k[i, s, :c, 5], kps[i, s]["octave"][:c]) and not k[i, s, c:].any() and not got["orb_descriptors"][i, s, c:].any()
        c = cnt[i, 0]
        assert np.array_equal(got["match_index"][i, :c], midx[i, :c]) and not got["match_index"][i, c:].any() and not got["triangulated_xyz"][i, c:].any()
    assert np.array_equal(got["db_best_id"], np.arange(P)) and got["ba_Hpp"].shape == (n, 36) and np.array_equal(got["sample_frames"], fr)
    with pytest.raises(AssertionError):           # the 64 MB bound
        write(str(tmp_path / "big"), P, cap, kps, desc, cnt, midx, midx, xyz, ok, lcd=(np.zeros((P, 40000), np.float32),) + lcd[1:])
