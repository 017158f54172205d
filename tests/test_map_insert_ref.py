"""tests/map_insert_ref.py — the literal walk of Map::InsertKeyFrame (src/map.cpp:17-48, :78-140) that the GPU tests of
myslam_backend_insert_keyframe_batch compare against — is itself checked here, on the CPU: against every map_insert_keyframe call of the package's
chain (<pkg>/chain.py) on its 44-frame run, and on the hand-made inputs of map_insert_ref.cases() for the property each was built for."""
import math

import numpy as np
import pytest

import backend_ref as br
import map_insert_ref as mi
from oracle_backend import OracleBackend


def _snapshot(c, tags, skip_kf=None):
    """the chain's active map as backend_ref containers, without the observations of `skip_kf` (KeyFrame::CreateKF has already appended them when
    Map::InsertKeyFrame is entered); a Feature keeps its tag for the whole run"""
    m = br.Map()
    m.kfs = {k: np.array(kf.pose, float) for k, kf in c.active_kfs.items()}
    for mid, mp in c.active_mps.items():
        q = br.MapPoint(mid, mp.pos, mp.outlier)
        for f in mp.obs:
            if f.kf is skip_kf:
                continue
            o = br.Obs(f.kf.id, f.x, f.y, f.outlier, tags.setdefault(id(f), len(tags)))
            q.obs.append(o)
            if any(g is f for g in mp.active_obs):
                q.active_obs.append(o)
        assert len(q.active_obs) == len(mp.active_obs)
        m.mps[mid] = q
    m.outlier_list = list(c.outlier_mps)
    return m


def _insert_of(c, kf, tags):
    feats, priors = [], {}
    for f in kf.feats:
        mp = f.live()
        if mp is None:
            feats.append((-1, (0.0, 0.0, 0.0), (f.x, f.y), tags.setdefault(id(f), len(tags)), f.outlier))
            continue
        feats.append((mp.id, tuple(mp.pos), (f.x, f.y), tags.setdefault(id(f), len(tags)), f.outlier))
        if mp.id not in c.active_mps and mp.id not in priors:               # GetObservations() of a map point that comes back
            priors[mp.id] = [(mp.id, g.kf.id, (g.x, g.y), tags.setdefault(id(g), len(tags)), g.outlier) for g in mp.obs if g.kf is not kf]
    return mi.Insert(kf.id, kf.pose, feats, [p for mid in sorted(priors) for p in priors[mid]])


def test_walk_reproduces_the_chains_map_insert(pkg, synth, oracle):
    """The 44-frame run of tests/test_backend_ref.py: the map before and after each of its 23 Map::InsertKeyFrame calls; the walk, given the chain's own
    distance, reproduces every after-state byte for byte.  What this run covers is asserted, so that nobody takes it for more: every new map-point id
    lies above the table's, no key-frame has two features on one map point."""
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(44)]
    cfg = {"numFeatures.trackingGood": 390}
    c = chain.Chain(OracleBackend(oracle, synth.calc_weights_handcrafted(), cfg, chain), pkg.api, synth.SEQ_K, frames, cfg=cfg)
    inner, calls, tags = c.map_insert_keyframe, [], {}

    def wrapped(kf):
        before, ins = _snapshot(c, tags, skip_kf=kf), _insert_of(c, kf, tags)
        inner(kf)
        calls.append((before, ins, _snapshot(c, tags)))

    c.map_insert_keyframe = wrapped
    c.run()
    assert len(calls) == len(c.kf_frames) == 23
    dist = lambda pk, pn, row: chain.se3_log_norm(chain.mm(chain.T_of(pk), chain.T_inv(chain.T_of(pn))))
    branches, middle, duplicate = [], 0, 0
    for before, ins, after in calls:
        ids = [f[0] for f in ins.feats if f[0] >= 0]
        new = sorted(set(i for i in ids if i not in before.mps))
        middle += int(bool(new) and bool(before.mps) and new[0] < max(before.mps))
        duplicate += int(len(set(ids)) != len(ids))
        n_kf = len(before.kfs)
        rep = mi.insert_walk(before, ins, c.window, 0.2, dist)
        assert rep["status"] == mi.OK
        got, want = br.pack(before), br.pack(after)
        for k in br.TABLES:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        assert (rep["removed_kf_id"] >= 0) == (n_kf + 1 > c.window)
        if rep["branch"]:
            branches.append(rep["branch"])
        rows = rep["feat_row"][[i for i, f in enumerate(ins.feats) if f[0] >= 0]]
        assert len(set(rows.tolist())) == len(rows) and (got["obs_kf"][rows] == len(got["kf_id"]) - 1).all()
    assert len(branches) >= 10 and set(branches) == {"nearest", "farthest"}
    assert middle == 0 and duplicate == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return mi.cases()


@pytest.fixture(scope="module")
def oracle_dist(oracle):
    def dist(pk, pn, row):
        d = oracle.se3_log(oracle.se3_compose(pk, pn, invert_b=True))
        s = 0.0
        for k in range(6):
            s += d[k] * d[k]
        return math.sqrt(s)
    return dist


def _run(case, dist):
    m = case["m"].clone()
    rep = mi.insert_walk(m, case["ins"], case["window"], case["th"], dist)
    return m, rep


def test_every_case_walks_and_keeps_the_tables_well_formed(cases, oracle_dist):
    for name, case in cases.items():
        m, rep = _run(case, oracle_dist)
        assert rep["status"] == case.get("status", mi.OK), name
        t = br.pack(m)
        assert np.all(np.diff(t["kf_id"]) > 0) and np.all(np.diff(t["mp_id"]) > 0) and np.all(np.diff(t["obs_mp"]) >= 0), name
        if rep["status"] != mi.OK:
            before = br.pack(case["m"])
            assert all(t[k].tobytes() == before[k].tobytes() for k in br.TABLES), name
            assert (rep["feat_row"] == -1).all() and (rep["mp_new_row"] == -1).all() and (rep["dis"] == -1).all() and rep["removed_kf_row"] == -1
            continue
        new_row = len(t["kf_id"]) - 1
        assert t["kf_id"][new_row] == case["ins"].kf_id
        for f, (mid, pos, uv, tag, outlier) in enumerate(case["ins"].feats):
            r = rep["feat_row"][f]
            if mid < 0:
                assert r == -1, name
                continue
            assert t["mp_id"][t["obs_mp"][r]] == mid and t["obs_kf"][r] == new_row and t["obs_tag"][r] == tag, name
            assert t["obs_flags"][r] == br.ACTIVE | (br.OUTLIER if outlier else 0), name
            assert r + 1 == len(t["obs_mp"]) or t["obs_mp"][r + 1] != t["obs_mp"][r] or t["obs_kf"][r + 1] == new_row, (name, "the END of its segment")
        assert (t["obs_kf"][t["obs_flags"] & br.ACTIVE != 0] >= 0).all(), name


def test_where_new_map_points_land(cases, oracle_dist):
    table = sorted(cases["new_below"]["m"].mps)
    for name, where in (("new_below", lambda new: max(new) < table[0]), ("new_between", lambda new: table[0] < min(new) and max(new) < table[-1]),
                        ("new_above", lambda new: min(new) > table[-1]),
                        ("interleaved", lambda new: min(new) < table[0] and max(new) > table[-1] and any(table[0] < i < table[-1] for i in new))):
        for suffix in ("", "_removal"):
            case = cases[name + suffix]
            new = [f[0] for f in case["ins"].feats if f[0] >= 0 and f[0] not in case["m"].mps]
            assert new and where(new), name
            m, rep = _run(case, oracle_dist)
            for f, feat in enumerate(case["ins"].feats):                    # the position of a new point is its first feature's
                if feat[0] in new and [g[0] for g in case["ins"].feats].index(feat[0]) == f:
                    assert np.array_equal(m.mps[feat[0]].pos, np.array(feat[1])) and not m.mps[feat[0]].outlier
            assert (rep["removed_kf_row"] >= 0) == bool(suffix)
    for name, mid, n in (("all_on_one_table_id", 106, 5), ("all_on_one_new_id", 107, 5)):
        m, rep = _run(cases[name], oracle_dist)
        rows = rep["feat_row"]
        assert len(rows) == n and (np.diff(rows) == 1).all() and [o.tag for o in m.mps[mid].obs[-n:]] == [f[3] for f in cases[name]["ins"].feats]
    m, rep = _run(cases["two_and_three_on_one_id"], oracle_dist)
    assert [len(m.mps[i].active_obs) - len(cases["two_and_three_on_one_id"]["m"].mps[i].active_obs) for i in (103, 109)] == [2, 3]
    assert [len(m.mps[i].obs) for i in (107, 120)] == [3, 2]
    before = br.pack(cases["all_without_map_point"]["m"])
    m, rep = _run(cases["all_without_map_point"], oracle_dist)
    after = br.pack(m)
    assert (rep["feat_row"] == -1).all() and all(after[k].tobytes() == before[k].tobytes() for k in br.TABLES if not k.startswith("kf_"))
    m, rep = _run(cases["feature_on_outlier_map_point"], oracle_dist)
    assert m.mps[106].outlier and m.mps[106].obs[-1].kf == 9 and rep["feat_row"][0] >= 0


def test_prior_rows_and_outlier_ids(cases, oracle_dist):
    for name, gone in (("prior_rows", None), ("prior_rows_removal", 8)):
        case = cases[name]
        m, rep = _run(case, oracle_dist)
        assert rep["removed_kf_id"] == (gone if gone is not None else -1)
        seg = m.mps[104].obs
        assert [o.tag for o in seg[:3]] == [902, 903, 904] and [o.kf for o in seg[3:]] == [9, 9] and len(m.mps[104].active_obs) == 2
        t = br.pack(m)
        rows = np.nonzero(t["mp_id"][t["obs_mp"]] == 104)[0][:3]
        kf_of = lambda k: sorted(m.kfs).index(k) if k in m.kfs else -1
        assert t["obs_kf"][rows].tolist() == [kf_of(o.kf) for o in seg[:3]] and (t["obs_flags"][rows] & br.ACTIVE == 0).all()
        assert (t["obs_kf"][rows] < 0).sum() == (2 if gone is not None else 1)       # outside the window, and the victim itself
        assert 901 not in [o.tag for o in m.mps[103].obs] and 105 not in m.mps       # an id in the table, an id no feature names
    for name in ("outlier_ids", "outlier_ids_removal"):
        case = cases[name]
        assert 103 in case["m"].mps and 112 in case["m"].mps and 999 not in case["m"].mps and not case["m"].mps[103].outlier
        m, rep = _run(case, oracle_dist)
        assert m.mps[103].outlier and 999 not in m.mps and not m.mps[200].outlier
        assert all(mp.outlier == (i in (103, 112)) for i, mp in m.mps.items())


def test_window_not_exceeded(cases, oracle_dist):
    case = cases["window_not_exceeded"]
    assert not case["m"].mps[104].active_obs
    m, rep = _run(case, oracle_dist)
    assert len(m.kfs) == case["window"] and 104 in m.mps and not m.mps[104].active_obs
    assert rep["removed_kf_row"] == -1 and (rep["dis"] == -1).all() and (rep["mp_new_row"] >= 0).all()


def test_the_rule_and_its_corners(cases, oracle_dist):
    for name, case in cases.items():
        if "victim_row" not in case:
            continue
        m, rep = _run(case, oracle_dist)
        assert rep["removed_kf_row"] == case["victim_row"], (name, rep["dis"])
        before = br.pack(case["m"])
        assert rep["removed_kf_id"] == before["kf_id"][case["victim_row"]] and rep["removed_kf_id"] not in m.kfs
        if "exact" in case:                                                 # pure translations by binary fractions: the oracle's distances are exact
            assert rep["dis"].tolist() == case["exact"], (name, rep["dis"])
        if case.get("gaps"):                                                # competing distances stand 1e-6 apart, from each other and from the threshold
            d = np.sort(np.concatenate([rep["dis"], [case["th"]]]))
            assert (np.diff(d) >= 1e-6 * d[1:]).all(), (name, d)
            assert set(before["obs_kf"].tolist()) >= set(range(len(before["kf_id"])))         # rows of every key-frame: the renumbering is seen
        after = br.pack(m)
        assert not (after["obs_flags"][after["obs_kf"] < 0] & br.ACTIVE).any(), name
    asc, desc = _run(cases["ascending"], oracle_dist)[1], _run(cases["descending"], oracle_dist)[1]
    assert asc["branch"] == "farthest" and min(asc["dis"]) < cases["ascending"]["th"]           # the `else if`: 0.0625 never became the minimum
    assert desc["branch"] == "nearest"
    assert _run(cases["on_the_threshold"], oracle_dist)[1]["branch"] == "farthest" and cases["on_the_threshold"]["th"] in cases["on_the_threshold"]["exact"]
    rep = _run(cases["all_nan_without_key_frame_0"], oracle_dist)[1]
    assert rep["status"] == mi.INVALID and 0 not in cases["all_nan_without_key_frame_0"]["m"].kfs


def test_sized_cases_have_their_sizes(cases, oracle_dist):
    for n in (0, 1, 511, 512, 513, 1025):
        assert len(br.rows_of(cases["obs_%d" % n]["m"])) == n
    for n in (0, 1, 64, 65, 513):
        assert len(cases["feat_%d" % n]["ins"].feats) == n
    for n in (1, 512, 513):
        assert len(cases["mp_%d" % n]["m"].mps) == n
    left = 0
    for name in ("obs_1025", "mp_513", "feat_513"):
        m, rep = _run(cases[name], oracle_dist)
        assert rep["status"] == mi.OK and rep["removed_kf_row"] >= 0
        left += int((rep["mp_new_row"] < 0).sum())
    assert left > 0                                                         # map points leave in the large cases


def test_pack_inputs_round_trip(cases):
    case = cases["prior_rows"]
    p = mi.pack_inputs([case["ins"], cases["outlier_ids"]["ins"]], 7, 6, 4)
    assert p["n_feat"].tolist() == [4, 2] and p["n_prior"].tolist() == [5, 0] and p["n_outlier"].tolist() == [0, 3]
    assert p["feat_mp_id"][0, :4].tolist() == [104, 103, 104, 200] and (p["feat_mp_id"][0, 4:] == -66).all()
    assert p["prior_flags"][0, :5].tolist() == [0, br.OUTLIER, 0, 0, 0] and p["outlier_mp_id"][1, :3].tolist() == [103, 999, 112]
    assert p["feat_mp_id"].dtype == np.int64 and p["feat_uv"].dtype == np.float32 and p["feat_flags"].dtype == np.uint8 and p["new_kf_pose"].shape == (2, 7)
