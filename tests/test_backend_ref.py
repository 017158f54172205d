"""tests/backend_ref.py — the literal walk of Backend::OptimizeActiveMap (src/backend.cpp:126-266, src/map.cpp:126-175) that the GPU tests of
myslam_backend_optimize_batch compare against — is itself checked here, on the CPU: its graph build against the library's host function
(myslam_ba_flatten_window), and the whole walk against the package's chain (<pkg>/chain.py) run through the oracle back end."""
import numpy as np
import pytest

import backend_ref as br
from oracle_backend import OracleBackend


@pytest.fixture(scope="module")
def api_host(pkg):
    import os
    if not os.path.exists(pkg.api.LIB_PATH):
        pkg.build_library()
    return pkg.api


@pytest.mark.parametrize("seed", range(8))
def test_walk_flat_window_is_the_host_functions(api_host, synth, seed):
    m, _, kinds = br.make_map(synth, 0x300 + seed, n_kf=6, n_mp=60)
    assert br.validate(m)
    flat, edge_objs, slot_mps = br.flatten(m)
    args, active_rows = br.host_flatten_args(m)
    host = api_host.ba_flatten_window(*args)
    assert br.same_flat(flat, host, active_rows)
    t = br.pack(m)                                           # the tables say the same as the containers
    assert np.all(np.diff(t["kf_id"]) > 0) and np.all(np.diff(t["mp_id"]) > 0) and np.all(np.diff(t["obs_mp"]) >= 0)
    assert np.all(t["obs_kf"][t["obs_flags"] & br.ACTIVE != 0] >= 0)
    edge = ((t["obs_flags"] & 3) == br.ACTIVE) & (t["mp_outlier"][t["obs_mp"]] == 0)
    assert np.array_equal(np.nonzero(edge)[0], flat["edge_src"])
    first = np.searchsorted(t["obs_mp"], flat["pt_src"])
    assert np.array_equal((t["obs_kf"][first] < 0).astype(np.uint8), flat["fixed"])
    # the map holds every kind of row the tables can hold
    assert {"fixed", "normal"} <= set(kinds.values()) and 0 < flat["fixed"].sum() < len(flat["fixed"])
    assert len(flat["edge_src"]) < len(t["obs_mp"]) and (t["obs_flags"] & br.OUTLIER).any() and (t["obs_kf"] < 0).any()
    assert ((t["obs_flags"] & br.ACTIVE == 0) & (t["obs_kf"] >= 0)).any()


def test_make_map_has_every_kind_over_the_seeds(synth):
    kinds = set()
    for seed in range(8):
        kinds |= set(br.make_map(synth, 0x300 + seed)[2].values())
    assert kinds == {"outlier_empty", "outlier", "inactive", "pair", "fixed", "normal"}


def _snapshot(c, tags):
    """the chain's active map as backend_ref containers; a Feature keeps its tag for the whole run"""
    m = br.Map()
    m.kfs = {k: np.array(kf.pose, float) for k, kf in c.active_kfs.items()}
    for mid, mp in c.active_mps.items():
        q = br.MapPoint(mid, mp.pos, mp.outlier)
        for f in mp.obs:
            o = br.Obs(f.kf.id, f.x, f.y, f.outlier, tags.setdefault(id(f), len(tags)))
            q.obs.append(o)
            if any(g is f for g in mp.active_obs):
                q.active_obs.append(o)
        assert len(q.active_obs) == len(mp.active_obs)       # every active observation is an observation
        m.mps[mid] = q
    m.outlier_list = list(c.outlier_mps)
    return m


def test_walk_reproduces_the_chains_back_end(pkg, synth, oracle):
    """The 44-frame short run of tests/test_chain_host.py: before and after each of its optimize_active_map calls (one per key-frame) the map is snapshot; the walk fed
    the logged solve results reproduces every after-state: table rows, outlier list, active set."""
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(44)]
    cfg = {"numFeatures.trackingGood": 390}
    c = chain.Chain(OracleBackend(oracle, synth.calc_weights_handcrafted(), cfg, chain), pkg.api, synth.SEQ_K, frames, cfg=cfg)
    inner, calls, tags = c.optimize_active_map, [], {}

    def wrapped():
        before, n = _snapshot(c, tags), len(c.log)
        inner()
        calls.append((before, [x for t, x in c.log[n:] if t == "ba"], _snapshot(c, tags)))

    c.optimize_active_map = wrapped
    c.run()
    assert len(calls) == len(c.kf_frames) >= 8              # one call per key-frame (backend.cpp:82-121)
    solved = removed = left = 0
    for before, ba, after in calls:
        assert len(ba) <= 1

        def solve(poses, pts, ep, el, eo, fixed, ba=ba):
            p2, x2, out, rn, chi = ba[0]
            assert len(out) == len(ep) and len(p2) == len(poses) and len(x2) == len(pts)
            return p2, x2, chi, out, int(rn[0]), int(rn[1])

        n_in = len(br.rows_of(before))
        rep = br.walk(before, solve)
        assert rep["status"] == (br.DONE if ba else br.EMPTY)
        got, want = br.pack(before), br.pack(after)
        for k in br.TABLES:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        assert before.outlier_list == after.outlier_list == [] or not ba
        assert sorted(before.mps) == sorted(after.mps) and sorted(before.kfs) == sorted(after.kfs)
        assert len(rep["obs_report"]) == n_in and n_in - int((rep["obs_report"] != 0).sum()) == len(got["obs_mp"])
        solved += bool(ba); removed += int((rep["obs_report"] == 1).sum()); left += int((rep["mp_report"] != 0).sum())
    assert solved >= 7 and removed > 0 and left > 0
