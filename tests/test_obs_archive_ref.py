"""tests/obs_archive_ref.py (the walk of myslam_obs_archive_*) against the object model of the reference's Map (tests/whole_map_model.py) over the 12
histories of tests/test_whole_map_model.HISTORIES, with the oracle's solve.  After every insert and every optimise the walk's live segments must be the
model's GetObservations() of every map point that is in all_mps and not in active_mps (key-frame ids, f32 pixels, tags, outlier bits), and before every
insert its prior arrays must be whole_map_model.priors_for.  The insert takes the WALK's priors, never the model's.  CPU only."""
import numpy as np
import pytest

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
import obs_archive_ref as oa
import test_whole_map_model as T
import whole_map_model as wm

# properties of the seeds, measured with the model
COUNTERS = dict(left_insert=177, left_optimize=81, left_optimize_culled=81, returned=123, left_again=58, erased=103)
LONGEST, MOST_PRIORS, MOST_LIVE = 16, 39, (231, 288)


def check_against_model(st, a, m):
    """-> None or what differs between the walk's live segments and the model's lists"""
    want = {mid: mp.obs for mid, mp in m.all_mps.items() if mid not in m.active_mps}
    got = dict(st.live(a))
    if sorted(got) != sorted(want):
        return "stored ids %s, the model's %s" % (sorted(got)[:6], sorted(want)[:6])
    for mid, rows in got.items():
        obs = want[mid]
        key_w = [(int(o.kf), np.float32(o.u).tobytes(), np.float32(o.v).tobytes(), int(o.tag), br.OUTLIER if o.outlier else 0) for o in obs]
        key_g = [(r[0], np.float32(r[1]).tobytes(), np.float32(r[2]).tobytes(), r[3], r[4]) for r in rows]
        if key_w != key_g:
            return "rows of map point %d" % mid
    return None


def replay(pkg, oracle, spec, faults=(), row_cap=1 << 20, stop_on_bad=False):
    """one history: the model, the walks of the back end's tables (w), of the map archive (a) and of the observation archive (st) side by side
    -> (the store, facts, mismatches)"""
    seed, window, n_kf, n_steps, extras = spec
    chain = pkg.chain
    m = wm.WholeMap(chain, window)
    w, a, st = br.Map(), mr.Archive(), oa.Store(row_cap)
    solve = T.oracle_solve(oracle)
    facts = dict(most_priors=0, events=[], stale=0, capacity_at=None)
    bad = []

    def check(where):
        why = check_against_model(st, a, m)
        if why is not None:
            bad.append((where, why))
        return why is not None and stop_on_bad

    n_ev = -1
    for ev in wm.history(seed, m, T.K, n_kf, n_steps, extras):
        n_ev += 1
        if ev.kind == "correct":
            m.correct(ev.rigid, ev.moves)
            for k in w.kfs:
                w.kfs[k] = m.all_kfs[k].pose.copy()
            for i, mp in w.mps.items():
                mp.pos = m.all_mps[i].pos.copy()
        elif ev.kind in ("insert", "refused", "capacity"):
            ins = ev.ins
            ps, priors = oa.prior_rows(st, [f[0] for f in ins.feats], sorted(w.mps), a)
            if st.err == oa.CAPACITY:
                assert ps == oa.CAPACITY and not priors
                break
            want = m.priors_for(ins.feats)
            if not faults:
                assert ps == oa.OK and oa.same_priors(priors, want), (spec, ins.kf_id)
            elif not oa.same_priors(priors, want):
                bad.append(("priors of key-frame %d" % ins.kf_id, "prior rows"))
                if stop_on_bad:
                    break
            facts["most_priors"] = max(facts["most_priors"], len(priors))
            if ev.kind == "capacity":                                       # the back end takes the key-frame, the map archive cannot: stale from here on
                ww = w.clone()
                ins.priors = priors
                rw = mi.insert_walk(ww, ins, window, 0.2, lambda pk, pn, row: m.dist(pk, pn))
                assert rw["status"] == mi.OK
                assert oa.update(st, oa.AFTER_INSERT, br.pack(ww), rw["status"], mr.CAPACITY, a) == oa.INVALID and st.err == oa.INVALID
                assert oa.prior_rows(st, [f[0] for f in ins.feats], sorted(ww.mps), a) == (oa.INVALID, [])
                facts["stale"] += 1
                continue
            rm = m.insert_keyframe(ins)                                     # sets ins.priors from the model's lists ...
            ins.priors = priors                                             # ... the walk of the tables takes the store's
            rw = mi.insert_walk(w, ins, window, 0.2, lambda pk, pn, row: m.dist(pk, pn))
            assert rw["status"] == rm["status"] == (mi.INVALID if ev.kind == "refused" else mi.OK)
            ms = mr.update(chain, a, mr.AFTER_INSERT, br.pack(w), rw["status"], outlier_ids=ins.outlier_ids)
            so = oa.update(st, oa.AFTER_INSERT, br.pack(w), rw["status"], ms, a, faults=faults)
            if so == oa.CAPACITY:
                facts["capacity_at"] = (n_ev, "insert", ins.kf_id)
                break
            if faults and so == oa.INVALID:
                bad.append(("insert of key-frame %d" % ins.kf_id, "refused by the walk itself"))
                break
            assert so == (oa.SKIPPED if ev.kind == "refused" else oa.UPDATED), (spec, so)
            if check("%s of key-frame %d" % (ev.kind, ins.kf_id)):
                break
        else:
            flat, edge_objs, slot_mps = br.flatten(m.active_map())
            sol = {}

            def poses():
                p2, x2, chi, out, _, _ = solve(np.stack([m.active_kfs[k].pose for k in sorted(m.active_kfs)]), np.stack([mp.pos for mp in slot_mps]),
                                               flat["edge_pose"], flat["edge_pt"], flat["edge_obs"], flat["fixed"])
                sol["x"] = {mp.id: x2[j] for j, mp in enumerate(slot_mps)}
                return {k: p2[i] for i, k in enumerate(sorted(m.active_kfs))}

            rm = m.optimize(ev.flags, poses, lambda: sol["x"])
            rw = br.walk(w, solve)
            assert rw["status"] == rm["status"]
            if rm["status"] == br.DONE:
                assert np.array_equal(rw["obs_report"], rm["obs_report"])
            ms = mr.update(chain, a, mr.AFTER_OPTIMIZE, br.pack(w), rw["status"], mp_report=rw["mp_report"], left_pos=rw["left_pos"])
            so = oa.update(st, oa.AFTER_OPTIMIZE, br.pack(w), rw["status"], ms, a, obs_report=rw["obs_report"], faults=faults)
            if so == oa.CAPACITY:
                facts["capacity_at"] = (n_ev, "optimize", max(m.all_kfs))
                break
            if faults and so == oa.INVALID:
                bad.append(("optimise after key-frame %d" % max(m.all_kfs), "refused by the walk itself"))
                break
            assert so == (oa.UPDATED if rm["status"] == br.DONE else oa.SKIPPED), (spec, so)
            if check("optimise after key-frame %d" % max(m.all_kfs)):
                break
    return st, facts, bad


@pytest.fixture(scope="module")
def runs(pkg, oracle):
    return {spec: replay(pkg, oracle, spec) for spec in T.HISTORIES}


@pytest.mark.parametrize("spec", T.HISTORIES, ids=lambda s: "seed%d_w%d" % s[:2])
def test_walk_equals_the_model_after_every_call(runs, spec):
    st, facts, bad = runs[spec]
    print(spec[0], st.seen, facts["most_priors"])
    assert not bad, bad[:3]
    assert facts["stale"] == ("capacity" in spec[4]) and facts["capacity_at"] is None
    assert st.n_reclaim == 0 and st.used >= st.seen["most_live"] and (st.used > 0 or spec[0] == 207)      # an unbounded pool only ever appends


def test_path_counters(runs):
    total = {k: sum(st.seen[k] for st, _, _ in runs.values()) for k in COUNTERS}
    print("paths over %d histories:" % len(runs), total)
    assert total == COUNTERS, total
    assert max(st.seen["longest"] for st, _, _ in runs.values()) == LONGEST
    assert max(f["most_priors"] for _, f, _ in runs.values()) == MOST_PRIORS
    most = {spec[0]: st.seen["most_live"] for spec, (st, _, _) in runs.items()}
    assert max(most.values()) == MOST_LIVE[0] == most[MOST_LIVE[1]], most


@pytest.mark.parametrize("fault", oa.FAULTS)
def test_stand_ins_are_refused(fault, pkg, oracle):
    refused = []
    for spec in T.HISTORIES:
        _, _, bad = replay(pkg, oracle, spec[:4] + (tuple(e for e in spec[4] if e != "capacity"),), faults=(fault,), stop_on_bad=True)
        if bad:
            refused.append((spec[0], bad[0]))
    print(fault, "refused on seeds", [s for s, _ in refused], "first:", refused[:1])
    assert len(refused) >= 1, fault


@pytest.mark.parametrize("seed, cap, stored", [(116, 47, 136), (149, 54, 173), (201, 67, 132)])
def test_reclaim_at_the_history_s_own_maximum(runs, pkg, oracle, seed, cap, stored):
    """row_cap = the most live rows the history ever holds: the walk must finish, by reclaiming; one row less and it names the event that overflows"""
    spec = next(s for s in T.HISTORIES if s[0] == seed)
    free = runs[spec][0]
    assert free.seen["most_live"] == cap and free.used == stored
    st, facts, bad = replay(pkg, oracle, spec, row_cap=cap)
    assert not bad and facts["capacity_at"] is None and st.n_reclaim >= 1 and st.seen["most_live"] == cap
    st, facts, bad = replay(pkg, oracle, spec, row_cap=cap - 1)
    assert facts["capacity_at"] is not None and st.err == oa.CAPACITY
    print(seed, "reclaims", st.n_reclaim, "capacity at", facts["capacity_at"])
