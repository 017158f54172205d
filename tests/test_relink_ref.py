"""The re-link rules of tests/relink_ref.py (plan, erased states, loop-store links, tracker landmarks: include/myslam_hip.h, RE-LINK) against the object
model of tests/relink_model.py, on the random histories of tests/test_whole_map_model.py with re-links placed after optimises and the histories
continued on the re-linked objects; and the rules' edges on hand-made tables.  CPU only."""
import numpy as np
import pytest

import relink_model as rm
import relink_ref as rr
from test_whole_map_model import HISTORIES, K


@pytest.fixture(scope="module")
def runs(pkg):
    return {spec: rr.run_history(pkg.chain, spec, K) for spec in HISTORIES}


@pytest.mark.parametrize("spec", HISTORIES, ids=lambda s: "seed%d_w%d" % s[:2])
def test_walks_equal_the_model_at_every_relink(runs, spec):
    cases, seen = runs[spec]                                                # run_history asserts every comparison
    assert cases, spec
    assert sum(c["plan"]["status"] == rr.DONE for c in cases) >= 1, spec


def test_path_counters(runs):
    total = {k: sum(seen[k] for _, seen in runs.values()) for k in rr.COUNTERS}
    print("\nre-link paths over %d histories, %d re-links: %s" % (len(runs), sum(len(c) for c, _ in runs.values()), total))
    assert all(total[k] > 0 for k in rr.COUNTERS), total
    assert max(c["count"] for cs, _ in runs.values() for c in cs) <= rr.MAX_PAIRS


def _tables():
    state = np.array([0, 0, 2, 1, 0, 0], np.uint8)
    cur = np.full(16, -1, np.int32); cur[:6] = [0, 1, -1, 0, 2, -1]
    loop = np.full(16, -1, np.int32); loop[:6] = [4, 5, 2, 3, -1, 4]
    return state, cur, loop


def _plan(pairs, state, cur, loop, outlier=None, status=rr.CORRECT_DONE, count=None, kf=9, out_cap=8, **kw):
    p = np.full((out_cap, 2), -9, np.int32); p[:len(pairs)] = pairs if pairs else np.zeros((0, 2))
    o = np.zeros(out_cap, np.uint8)
    if outlier:
        o[list(outlier)] = 1
    return rr.plan(p, len(pairs) if count is None else count, o, status, cur, loop, kf, state, len(state), out_cap=out_cap, **kw)


def test_plan_rule_edges():
    state, cur, loop = _tables()
    # merge 0 -> 4; feature 3 shares point 0 and follows; feature 2 adopts 5; feature 4's own point is erased: it adopts; loop features 2 (erased) and 4
    # (none) are skipped, only the erased one counts as dead; (0, 5): the feature's point is 4 by now, 4 == loop feature 5's point: the same point
    p = _plan([(0, 0), (2, 1), (4, 3), (1, 2), (1, 4), (0, 5)], state, cur, loop)
    assert p["status"] == rr.DONE and p["merge"] == [(0, 4)] and p["adopt"] == [(2, 5), (4, 3)] and p["report"] == [6, 1, 2, 1, 1, 4]
    assert p["target"].tolist() == [4, -1, -1, 3, 4, 5] and p["cur"][:6].tolist() == [4, 1, 5, 4, 3, -1]
    assert p["links"] == [(9, 0, 4), (9, 2, 5), (9, 3, 4), (9, 4, 3)]
    assert np.array_equal(cur[:6], [0, 1, -1, 0, 2, -1])                    # the input is not touched
    # a chain: (0, l=4) then (0, l=5) merges 4 into 5; target of 0 is 5
    p = _plan([(0, 0), (0, 1)], state, cur, loop)
    assert p["merge"] == [(0, 4), (4, 5)] and p["target"].tolist() == [5, -1, -1, -1, 5, 5] and p["cur"][:4].tolist() == [5, 1, -1, 5]
    # a loop point that was merged away is followed: loop feature 0 names 4, which went into 5
    p = _plan([(0, 1), (1, 5)], state, np.array([4, 1] + [-1] * 14, np.int32), loop)
    assert p["merge"] == [(4, 5), (1, 5)] and p["target"].tolist() == [-1, 5, -1, -1, 5, 5] and p["cur"][:2].tolist() == [5, 5]
    # adopt, then the adopted point is merged away: the adoption is null again and the feature adopts anew at its next pair
    cur2 = np.full(16, -1, np.int32); cur2[:3] = [-1, 4, -1]
    p = _plan([(0, 0), (1, 1), (0, 3)], state, cur2, loop)
    assert p["adopt"] == [(0, 4), (0, 3)] and p["merge"] == [(4, 5)] and p["cur"][:2].tolist() == [3, 5]
    p = _plan([(0, 0), (1, 1)], state, cur2, loop)
    assert p["adopt"] == [(0, 4)] and p["merge"] == [(4, 5)] and p["cur"][:2].tolist() == [-1, 5] and p["links"] == [(9, 0, -1), (9, 1, 5)]
    # outlier pairs are not walked; statuses that do not run
    p = _plan([(0, 0), (1, 1)], state, cur, loop, outlier=[0])
    assert p["merge"] == [(1, 5)] and p["report"][0] == 1
    for st in (rr.CORRECT_NOT_NEEDED, rr.CORRECT_SKIPPED, -1, -3, 7):
        p = _plan([(0, 0)], state, cur, loop, status=st)
        assert p["status"] == rr.SKIPPED and not p["merge"] and np.all(p["target"] == -1) and np.array_equal(p["cur"], cur)
    assert _plan([(0, 0)], state, cur, loop, status=rr.CORRECT_FUSED_ONLY)["merge"] == [(0, 4)]
    # refusals: counts, ids, slots — and an outlier pair is never looked at
    for bad in (dict(count=-1), dict(count=9), dict(kf=-1)):
        assert _plan([(0, 0)], state, cur, loop, **bad)["status"] == rr.INVALID
    for pr in ((16, 0), (-1, 0), (0, 16), (0, -1)):
        assert _plan([pr], state, cur, loop)["status"] == rr.INVALID
        assert _plan([pr, (0, 0)], state, cur, loop, outlier=[0])["status"] == rr.DONE
    for tab, f, v in (("cur", 0, 6), ("cur", 0, -2), ("loop", 0, 6), ("loop", 0, -2)):
        c2, l2 = cur.copy(), loop.copy()
        (c2 if tab == "cur" else l2)[f] = v
        assert _plan([(0, 0)], state, c2, l2)["status"] == rr.INVALID
        assert _plan([(1, 1)], state, c2, l2)["status"] == rr.DONE          # a slot no walked pair names is not judged
    assert _plan([], state, cur, loop)["report"] == [0] * 6


def test_map_relink_rule_edges():
    state = np.array([0, 1, 2, 0], np.uint8)
    st, s2 = rr.map_relink(state, [(0, 3), (1, 3)], 2, 4, rr.DONE)
    assert st == rr.MAP_UPDATED and s2.tolist() == [2, 2, 2, 0]
    st, s2 = rr.map_relink(state, [(0, 3), (1, 3)], 1, 4, rr.DONE)
    assert s2.tolist() == [2, 1, 2, 0]
    for status in (rr.SKIPPED, rr.INVALID):
        st, s2 = rr.map_relink(state, [(0, 3)], 1, 4, status)
        assert st == rr.MAP_SKIPPED and np.array_equal(s2, state)
    for merge, n in (([(4, 0)], 1), ([(0, 4)], 1), ([(-1, 0)], 1), ([(1, 1)], 1), ([(0, 3)], -1), ([(0, 3)] * 5, 5)):
        st, s2 = rr.map_relink(state, merge, n, 4, rr.DONE)
        assert st == rr.INVALID and np.array_equal(s2, state)


def test_set_links_rule_edges():
    s = rr.Store(8)
    s.put(10, [100, 101, 102, 103, 104], 5)
    s.put(20, [200, 201], 2)
    assert s.set_links([(10, 4, 7), (10, 5, 7), (10, -1, 7), (-3, 1, 7), (15, 0, 7), (20, 1, -1), (20, 0, -2)]) == 2
    assert s.gather(10)[:5].tolist() == [100, 101, 102, 103, 7] and s.gather(20)[:2].tolist() == [200, -1]
    pend = np.arange(8, dtype=np.int32)
    assert s.set_links([(30, 2, 5), (30, 8, 5), (10, 2, 6)], pending_id=30, pending=pend) == 2 and pend[2] == 5 and s.gather(10)[2] == 6
    assert s.set_links([(10, 1, 1), (10, 2, 2)], n=9, list_cap=1) == 1 and s.set_links([(10, 1, 1)], n=-2, list_cap=4) == 0
    # clear_links is set_links with -1
    a, b = rr.Store(8), rr.Store(8)
    for st in (a, b):
        st.put(10, [100, 101, 102], 3)
    assert a.clear_links([(10, 1), (11, 0)]) == b.set_links([(10, 1, -1), (11, 0, -1)]) == 1 and np.array_equal(a.gather(10), b.gather(10))


def _trk():
    return dict(ids_valid=1, ref_frame_id=6, next_frame_id=7, ref_kf_id=40, lm=np.array([0, 1, -1, 0, -1], np.int32), lm_id=np.array([500, 501], np.int64),
                lm_pos=np.array([[1., 2, 3], [4, 5, 6]]), lm_outl=np.array([0, 1], np.uint8))


def test_tracker_relink_rule_edges():
    mp_id = np.array([500, 501, 502, 503], np.int64)
    mp_pos = np.arange(12, dtype=float).reshape(4, 3) + 0.5
    state = np.array([2, 0, 1, 0], np.uint8)
    t = _trk()
    # features 0 and 3 share slot 0 and both moved to point 502 (listed: outlier flag); feature 2 adopts 501, which slot 1 carries; feature 4 adopts 503:
    # a new slot; an entry of another key-frame, a tag out of range
    st, hits, opened, shared = rr.tracker_relink(t, [(40, 0, 2), (40, 2, 1), (40, 3, 2), (40, 4, 3), (41, 1, 3), (40, 5, 3), (40, -1, 3)], mp_id, mp_pos, state, 3)
    assert (st, hits, opened, shared) == (rr.OK, 4, 1, 1)
    assert t["lm"].tolist() == [0, 1, 1, 0, 2] and t["lm_id"].tolist() == [502, 501, 503] and t["lm_outl"].tolist() == [1, 0, 0]
    assert np.array_equal(t["lm_pos"], mp_pos[[2, 1, 3]])
    # slot -1 drops the landmark; a full table refuses and keeps every byte; a slot out of range likewise
    t = _trk()
    assert rr.tracker_relink(t, [(40, 1, -1)], mp_id, mp_pos, state, 2)[:2] == (rr.OK, 1) and t["lm"].tolist() == [0, -1, -1, 0, -1]
    for entries, want in (([(40, 0, 2), (40, 4, 3)], rr.CAPACITY), ([(40, 0, 2), (40, 4, 4)], rr.INVALID), ([(40, 4, -2)], rr.INVALID)):
        t = _trk()
        assert rr.tracker_relink(t, entries, mp_id, mp_pos, state, 2)[0] == want
        assert all(np.array_equal(t[k], _trk()[k]) for k in ("lm", "lm_id", "lm_pos", "lm_outl"))
    # the guard: a stream that has stepped, or whose ids are not valid, keeps every byte
    for other in (dict(_trk(), next_frame_id=8), dict(_trk(), ids_valid=0)):
        assert rr.tracker_relink(other, [(40, 0, 2)], mp_id, mp_pos, state, 3)[:2] == (rr.OK, 0) and other["lm_id"].tolist() == [500, 501]
    # two adopting features on one new point share the new slot
    t = _trk()
    assert rr.tracker_relink(t, [(40, 2, 3), (40, 4, 3)], mp_id, mp_pos, state, 3)[1:] == (2, 1, 1) and t["lm"].tolist() == [0, 1, 2, 0, 2]


def test_model_refuses_a_merge_into_a_rowless_target(pkg):
    import backend_ref as br
    import whole_map_model as wm
    m = rm.RelinkMap(pkg.chain, 3)
    a, b = br.MapPoint(1, (0, 0, 5)), br.MapPoint(2, (0, 0, 6))
    m.all_mps = {1: a, 2: b}
    a.obs.append(wm.Obs(7, 1.0, 2.0, tag=0))
    m.adopted[(3, 5)] = b                                                   # the loop key-frame's feature adopted b in an earlier loop: b has no row
    with pytest.raises(rm.RowlessTarget):
        m.relink([(0, 5)], 7, 3)
    b.obs.append(wm.Obs(3, 1.0, 2.0, tag=5)); del m.adopted[(3, 5)]
    rep = m.relink([(0, 5)], 7, 3)
    assert rep["merges"] == [(1, 2)] and rep["moved"] == [(7, 0, 2)] and 1 in m.erased and m.link(7, 0) is b and len(b.obs) == 2


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the rows: whole histories with the walks of the back end's tables, the map archive and the observation archive beside the model

@pytest.fixture(scope="module")
def row_runs(pkg):
    return {spec: rr.replay_rows(pkg.chain, spec, K) for spec in HISTORIES}


@pytest.mark.parametrize("spec", HISTORIES, ids=lambda s: "seed%d_w%d" % s[:2])
def test_tables_segments_states_first_observers_and_stored_links_equal_the_model_after_every_event(row_runs, spec):
    out = row_runs[spec]                                                    # replay_rows asserts every comparison, after every event of the continued history
    assert out["capacity_at"] is None and out["checks"] >= 20 and out["cases"], spec
    assert out["first_kf_equals_loop_inputs"]                               # up to a history's first re-link the minimum rule and the list order agree


def test_row_path_counters(row_runs):
    total = {k: sum(o["seen"][k] for o in row_runs.values()) for k in rr.ROW_COUNTERS}
    print("\nre-link rows over %d histories, %d re-links: %s" % (len(row_runs), sum(len(o["cases"]) for o in row_runs.values()), total))
    assert all(total[k] > 0 for k in rr.ROW_COUNTERS if k != "reclaim"), total     # (a reclaim needs a pool at its limit: the test below)


@pytest.mark.parametrize("spec", HISTORIES[:12], ids=lambda s: "seed%d_w%d" % s[:2])
def test_first_kf_in_list_order_equals_loop_inputs_on_the_histories_without_a_relink(pkg, spec):
    out = rr.replay_rows(pkg.chain, spec, K, relinks=False)
    assert out["first_kf_equals_loop_inputs"] and not out["cases"] and out["checks"] >= 20


def test_reclaim_during_a_relink_and_capacity_one_row_below(pkg, row_runs):
    """row_cap = the most live rows a continued history ever holds: it must finish, reclaiming; for at least one history a reclaim falls into a
    re-link; one row below, the walk names the event that overflows"""
    in_relink = at_relink = 0
    for spec in HISTORIES:
        cap = row_runs[spec]["most_live"]
        if cap < 8:
            continue
        out = rr.replay_rows(pkg.chain, spec, K, row_cap=cap)
        assert out["capacity_at"] is None and out["st"].n_reclaim >= 1 and out["most_live"] == cap, spec
        in_relink += out["seen"]["reclaim"]
        low = rr.replay_rows(pkg.chain, spec, K, row_cap=cap - 1)
        assert low["capacity_at"] is not None, spec
        at_relink += low["capacity_at"][1] == "relink"
    print("\nreclaims that fell into a re-link:", in_relink, "; histories whose overflow one row below is a re-link:", at_relink)
    assert in_relink >= 1 and at_relink >= 1


def _store_and_archive():
    import map_archive_ref as mr
    import obs_archive_ref as oa
    a = mr.Archive()
    a.kf_id = [3, 5, 8]; a.kf_pose = [np.zeros(7)] * 3
    a.mp_id = [10, 11, 12, 13]; a.mp_state = [0, 0, 0, 0]; a.mp_pos = [np.zeros(3)] * 4
    row = lambda kf, tag, fl=0: (kf, np.float32(tag), np.float32(1.5), tag, fl)
    st = oa.Store.loaded(6, [(12, [row(3, 20), row(5, 21)]), (13, [row(3, 30, 2)])], [10, 11], [[row(5, 1), row(8, 2)], [row(8, 3)]])
    return st, a, row


def test_stage_rule_edges():
    st, a, row = _store_and_archive()
    # 10 (table) -> 12 (stored), then 12 -> 11 (table): the chain is flat in the staging, 10's rows stand behind 12's in 11's list
    target = np.array([1, 1, 1, -1], np.int32)
    s = rr.stage(st, a, [(0, 2), (2, 1)], target, rr.DONE)
    assert s["status"] == rr.DONE and s["merges"] == [(10, 11, 2), (12, 11, 2)]
    assert [(r[0], r[3], r[5], r[6], r[7]) for r in s["rows"]] == [(5, 1, 11, 3, 1), (8, 2, 11, 4, 1), (3, 20, 11, 1, 1), (5, 21, 11, 2, 1)]
    assert rr.moved_links(s) == [(5, 1, 1), (8, 2, 1), (3, 20, 1), (5, 21, 1)]
    # the table holds 3 rows and ends with 1 + 4: obs_cap 5 holds it, 4 does not; nothing is sticky
    assert rr.stage(st, a, [(0, 2), (2, 1)], target, rr.DONE, be_obs_cap=5)["status"] == rr.DONE
    assert rr.stage(st, a, [(0, 2), (2, 1)], target, rr.DONE, be_obs_cap=4)["status"] == rr.CAPACITY and st.err == 0
    # 10 (table) -> 13 (stored): 1 + 2 rows outside plus 12's 2 = 5 of row_cap 6; with row_cap 4 it is refused
    t2 = np.array([3, -1, -1, 3], np.int32)
    assert rr.stage(st, a, [(0, 3)], t2, rr.DONE)["status"] == rr.DONE
    st.row_cap = 4
    assert rr.stage(st, a, [(0, 3)], t2, rr.DONE)["status"] == rr.CAPACITY
    st.row_cap = 6
    # refusals: a slot out of range, a point merged into itself, an erased point, a target that does not stand; statuses that do not run; a sticky error
    for merge, tg in (([(0, 4)], target), ([(-1, 1)], target), ([(1, 1)], target), ([(0, 2)], np.array([2, -1, 1, -1], np.int32)), ([(0, 2)], np.array([-1] * 4, np.int32))):
        assert rr.stage(st, a, merge, tg, rr.DONE)["status"] == rr.INVALID
    a.mp_state[2] = 2
    assert rr.stage(st, a, [(0, 2), (2, 1)], target, rr.DONE)["status"] == rr.INVALID
    a.mp_state[2] = 0
    assert rr.stage(st, a, [(0, 2)], target, rr.SKIPPED)["status"] == rr.SKIPPED and rr.stage(st, a, [(0, 2)], target, rr.INVALID)["status"] == rr.SKIPPED
    st.err = -3
    assert rr.stage(st, a, [(0, 2)], target, rr.DONE)["status"] == -3


def test_first_kf_is_the_front_of_the_list_not_the_lowest_observer():
    st, a, row = _store_and_archive()
    # 11's own row is of key-frame 8; the rows it received are of 5 and 3: the front stays 8 (archive row 2); the minimum rule would say 3 (row 0)
    st.t_rows[1] = [row(8, 3), row(5, 40), row(3, 41)]
    assert rr.first_kf(st, a).tolist() == [1, 2, 0, 0]
    st.t_rows[1] = st.t_rows[1][1:]                                         # the front is culled: the next row IN LIST ORDER is of key-frame 5, not of 3
    assert rr.first_kf(st, a).tolist() == [1, 1, 0, 0]
    a.mp_state[3] = 2; st.seg[12] = (0, 0)
    assert rr.first_kf(st, a).tolist() == [1, 1, -1, -1]


def test_obs_cap_one_row_below_on_the_histories(pkg):
    """a recorded re-link whose table ends with MORE rows than it had (rows come out of the store into a target of the table): the stage refuses at
    obs_cap one row below what the table needs and serves at exactly that; the back end's own check answers the same for rows staged against a
    larger cap (on the device the stage decides first, so that branch is a second line)"""
    import copy
    import backend_ref as br
    found = 0
    for spec in HISTORIES:
        for c in rr.replay_rows(pkg.chain, spec, K, record=True)["cases"]:
            if c["plan"]["status"] != rr.DONE:
                continue
            p, a, st = c["plan"], c["a_before"], c["st_before"]
            free = rr.stage(st, a, p["merge"], p["target"], rr.DONE)
            w = c["w_before"].clone()
            before = len(br.pack(w)["obs_mp"])
            assert rr.backend_relink(w, free)["status"] == rr.OK
            need = len(br.pack(w)["obs_mp"])
            if need <= before:
                continue
            found += 1
            assert rr.stage(st, a, p["merge"], p["target"], rr.DONE, be_obs_cap=need - 1)["status"] == rr.CAPACITY and st.err == 0
            assert rr.stage(st, a, p["merge"], p["target"], rr.DONE, be_obs_cap=need)["status"] == rr.DONE
            w2 = c["w_before"].clone()
            t0 = br.pack(w2)
            r = rr.backend_relink(w2, free, obs_cap=need - 1)
            assert r["status"] == rr.CAPACITY and (r["mp_new_row"] == -1).all() and all(np.array_equal(br.pack(w2)[k], t0[k]) for k in br.TABLES)
            assert rr.backend_relink(copy.deepcopy(c["w_before"]), free, obs_cap=need)["status"] == rr.OK
            assert rr.stage(st, a, p["merge"], p["target"], rr.DONE, stage_cap=len(free["rows"]) - 1)["status"] == rr.CAPACITY
    print("\nre-links that grow the table:", found)
    assert found >= 1
