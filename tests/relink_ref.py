"""The calls of include/myslam_hip.h's RE-LINK section in plain Python, on tables shaped as the device's: plan (myslam_loop_relink_plan_batch),
map_relink (myslam_map_relink_batch), Store.set_links (myslam_loop_store_set_links_batch) and tracker_relink (myslam_tracker_relink_batch); and
run_history, which holds them against the object model of tests/relink_model.py on the random histories of tests/whole_map_model.py, with a re-link
placed after optimises of a history that is CONTINUED afterwards on the re-linked objects.  A feature's index is its tag, as in
tests/link_upkeep_ref.py.  Test helper, no GPU."""
import numpy as np

import link_upkeep_ref as lu
import relink_model as rm
import whole_map_model as wm

OK, INVALID, CAPACITY = 0, -1, -3
DONE, SKIPPED = 0, 1                                # MYSLAM_RELINK_*
CORRECT_DONE, CORRECT_NOT_NEEDED, CORRECT_SKIPPED, CORRECT_FUSED_ONLY = 0, 1, 2, 3
MAP_UPDATED, MAP_SKIPPED = 0, 1
FEAT_CAP = lu.FEAT_CAP
OUT_CAP = 40                                        # pairs of one loop: at most 32 are made
MAX_PAIRS = 32
COUNTERS = ("merge_target_outside_table", "merge_target_inside_table", "adopt", "same_point", "chain_merge", "dead_loop_point", "skipped_or_not_needed",
            "adopted_then_merged_away", "outlier_pairs", "tracker_new_slot", "tracker_shared_slot", "links")


def lock(slot, mp_state):
    """mpMapPoint.lock() of a table entry: None for no slot and for an erased point"""
    return None if slot < 0 or mp_state[slot] == 2 else int(slot)


def plan(pairs, count, outlier, correct_status, cur, loop, cur_kf_id, mp_state, n_mp, out_cap=OUT_CAP, point_cap=None):
    """-> dict(status, merge [(from, to)], adopt [(feature, slot)], target (n_mp), cur (the table afterwards), links [(kf id, feature, slot)], report).
    pairs: out_cap x 2, outlier: out_cap, cur / loop: feat_cap each; nothing given is changed"""
    feat_cap = len(cur)
    empty = lambda st: dict(status=st, merge=[], adopt=[], target=np.full(max(0, min(n_mp, point_cap if point_cap is not None else n_mp)), -1, np.int32),
                            cur=np.array(cur, np.int32), links=[], report=[0] * 6)
    if correct_status not in (CORRECT_DONE, CORRECT_FUSED_ONLY):
        return empty(SKIPPED)
    if n_mp < 0 or (point_cap is not None and n_mp > point_cap) or count < 0 or count > out_cap or cur_kf_id < 0:
        return empty(INVALID)
    walk = [(int(pairs[i][0]), int(pairs[i][1])) for i in range(count) if not outlier[i]]
    for cf, lf in walk:
        if not (0 <= cf < feat_cap and 0 <= lf < feat_cap) or not (-1 <= cur[cf] < n_mp) or not (-1 <= loop[lf] < n_mp):
            return empty(INVALID)
    cur = np.array(cur, np.int32)
    into = {}                                       # a merged point -> the point it went into
    touched, adopted = set(), set()

    def end(s):
        while s in into:
            s = into[s]
        return s

    merge, adopt, same, dead = [], [], 0, 0
    for cf, lf in walk:
        l = lock(int(loop[lf]), mp_state)
        if l is None:
            dead += loop[lf] >= 0
            continue
        l = end(l)
        c = lock(int(cur[cf]), mp_state)
        if c is not None:
            c = (None if c in into else c) if cf in adopted else end(c)
        if c is None:
            cur[cf] = l; adopted.add(cf); adopt.append((cf, l)); touched.add(l)
        elif c == l:
            same += 1
        else:
            merge.append((c, l)); into[c] = l; touched |= {c, l}
    target = np.full(n_mp, -1, np.int32)
    for s in touched:
        target[s] = end(s)
    links = []
    for f in range(feat_cap):
        e = int(cur[f])
        moved = 0 <= e < n_mp and e in into
        if f in adopted:
            if moved:
                cur[f] = -1
            links.append((int(cur_kf_id), f, int(cur[f])))
        elif moved:
            cur[f] = end(e)
            links.append((int(cur_kf_id), f, int(cur[f])))
    return dict(status=DONE, merge=merge, adopt=adopt, target=target, cur=cur, links=links, report=[len(walk), len(merge), len(adopt), same, int(dead), len(links)])


def map_relink(mp_state, merge, n_merge, merge_cap, plan_status):
    """-> (status, the states afterwards)"""
    state = np.array(mp_state, np.uint8)
    if plan_status != DONE:
        return MAP_SKIPPED, state
    if n_merge < 0 or n_merge > merge_cap or any(not (0 <= a < len(state) and 0 <= b < len(state)) or a == b for a, b in merge[:n_merge]):
        return INVALID, state
    for a, _ in merge[:n_merge]:
        state[a] = 2
    return MAP_UPDATED, state


class Store(lu.Store):
    def set_links(self, entries, n=None, list_cap=None, pending_id=None, pending=None):
        """entries: [(kf id, tag, slot)]: clear_links with a value; an entry with a slot below -1 is ignored"""
        assert (pending_id is None) == (pending is None)
        if n is not None:
            entries = entries[:max(0, min(int(n), int(list_cap)))]
        hits = 0
        for kf_id, tag, slot in entries:
            if kf_id < 0 or tag < 0 or slot < -1:
                continue
            if pending is not None and kf_id == pending_id and tag < self.feat_cap:
                pending[tag] = slot
                hits += 1
            elif kf_id in self.ids:
                t = self.tables[self.ids.index(kf_id)]
                if tag < len(t):
                    t[tag] = slot
                    hits += 1
        return hits


def tracker_relink(trk, entries, mp_id, mp_pos, mp_state, lm_cap, n=None, list_cap=None):
    """trk: dict(ids_valid, ref_frame_id, next_frame_id, ref_kf_id, lm: feature -> landmark slot, lm_id / lm_pos / lm_outl by landmark slot), changed in
    place unless refused.  entries: [(kf id, tag, slot)].  -> (status, naming entries, new landmark slots, features that took a slot already there)"""
    if not trk["ids_valid"] or trk["ref_frame_id"] != trk["next_frame_id"] - 1:
        return OK, 0, 0, 0
    if n is not None:
        entries = entries[:max(0, min(int(n), int(list_cap)))]
    mine = [(tag, slot) for kf_id, tag, slot in entries if kf_id == trk["ref_kf_id"] and 0 <= tag < len(trk["lm"])]
    if any(slot < -1 or slot >= len(mp_id) for _, slot in mine):
        return INVALID, 0, 0, 0
    lm, ids, src = trk["lm"].copy(), [int(v) for v in trk["lm_id"]], {}
    n0, shared = len(ids), 0
    for tag, slot in mine:
        if slot < 0:
            lm[tag] = -1
            continue
        pid = int(mp_id[slot])
        L = int(lm[tag])
        if L >= 0:
            ids[L] = pid; src[L] = slot
            continue
        if pid in ids:
            L = ids.index(pid); shared += 1
        else:
            if len(ids) >= lm_cap:
                return CAPACITY, 0, 0, 0
            L = len(ids); ids.append(pid)
        lm[tag] = L; src[L] = slot
    pos = np.concatenate([np.array(trk["lm_pos"], float).reshape(-1, 3), np.zeros((len(ids) - n0, 3))])
    outl = np.concatenate([np.array(trk["lm_outl"], np.uint8), np.zeros(len(ids) - n0, np.uint8)])
    for L, slot in src.items():
        pos[L] = mp_pos[slot]; outl[L] = mp_state[slot] == 1
    trk.update(lm=lm, lm_id=np.array(ids, np.int64), lm_pos=pos, lm_outl=outl)
    return OK, len(mine), len(ids) - n0, shared


# ---------------------------------------------------------------------------------------------------------------------------------------------
# against the object model

def archive_of(m):
    """the map archive's point tables as the model implies them: every id ever inserted ascending, state 2 erased / 1 listed / 0, positions"""
    ids = sorted(set(m.all_mps) | set(m.erased))
    listed = set(m.outlier_mps)
    state = np.array([2 if i not in m.all_mps else (1 if i in listed else 0) for i in ids], np.uint8)
    pos = np.array([m.all_mps[i].pos if i in m.all_mps else (0.0, 0.0, 0.0) for i in ids], float).reshape(-1, 3)
    return np.array(ids, np.int64), state, pos


def table_of(m, mp_ids, kf_id, feats, stale=True):
    """key-frame kf_id's feature -> archive-slot table by tag, from the model: the slot of the feature's point; with `stale` a feature whose own point
    was erased keeps naming its slot (a stored table before myslam_map_filter_landmarks_batch)"""
    at = {int(v): i for i, v in enumerate(mp_ids)}
    row = np.full(FEAT_CAP, -1, np.int32)
    links = m.links(kf_id)
    for mid, _, _, tag, _ in feats:
        if tag in links:
            row[tag] = at[links[tag].id]
        elif stale and mid >= 0 and mid in m.erased:
            row[tag] = at[int(mid)]
    return row


def make_pairs(rng, m, cur_kf, cur_feats, loop_kf, loop_feats):
    """up to MAX_PAIRS (current tag, loop tag): random ones, a chain (c, l1), (c, l2), a repeated pair, features without a point on both sides, and a
    pair on one point when the two key-frames share one"""
    cl, ll = m.links(cur_kf), m.links(loop_kf)
    ctags, ltags = [f[3] for f in cur_feats], [f[3] for f in loop_feats]
    pairs = []
    shared = [(c, l) for c in sorted(cl) for l in sorted(ll) if cl[c] is ll[l]]
    if shared:
        pairs.append(shared[int(rng.integers(len(shared)))])
    linked_l = sorted(ll)
    if len(linked_l) >= 2 and cl:
        c = sorted(cl)[int(rng.integers(len(cl)))]
        l1, l2 = (linked_l[i] for i in rng.choice(len(linked_l), 2, replace=False))
        pairs += [(c, l1), (c, l2)]
    free_c = [t for t in ctags if t not in cl]
    for t in free_c[:2]:                                                    # adopt; the second one twice (the later pair finds it adopted)
        if linked_l:
            pairs.append((t, linked_l[int(rng.integers(len(linked_l)))]))
    if free_c and len(linked_l) >= 2:                                       # adopt a point, then merge that point away: the adoption dies with it
        a, b = (linked_l[i] for i in rng.choice(len(linked_l), 2, replace=False))
        other = [c for c in sorted(cl) if cl[c] is not ll[a] and cl[c] is not ll[b]]
        if other:
            pairs += [(free_c[-1], a), (other[0], b), (other[0], a)]
    n = int(rng.integers(4, 12))
    for _ in range(n):
        pairs.append((ctags[int(rng.integers(len(ctags)))], ltags[int(rng.integers(len(ltags)))]))
    if pairs:
        pairs.append(pairs[int(rng.integers(len(pairs)))])
    order = rng.permutation(len(pairs)) if rng.random() < 0.3 else np.arange(len(pairs))
    return [pairs[i] for i in order][:MAX_PAIRS]


def tracker_of(m, cur_kf, feats, frame, lm_cap):
    """the tracker right after key-frame cur_kf was made: one landmark slot per distinct id its features name, in order of first naming"""
    ids, n_feat = lu.feat_ids_by_tag(feats)
    links = m.links(cur_kf)
    lm_id, lm = [], np.full(n_feat, -1, np.int32)
    for mid, _, _, tag, _ in feats:
        if tag in links:                                                    # culled links are already cleared (LINK UPKEEP)
            if links[tag].id not in lm_id:
                lm_id.append(links[tag].id)
            lm[tag] = lm_id.index(links[tag].id)
    return dict(ids_valid=1, ref_frame_id=frame, next_frame_id=frame + 1, ref_kf_id=cur_kf, lm=lm, lm_id=np.array(lm_id, np.int64),
                lm_pos=np.array([m.all_mps[i].pos for i in lm_id], float).reshape(-1, 3), lm_outl=np.array([m.all_mps[i].outlier for i in lm_id], np.uint8))


def run_history(chain, spec, K, every=2, lm_slack=3):
    """One history on the model alone (the optimiser's numbers do not matter to the re-link: the constructed flags are taken as the outliers and nothing
    moves), a re-link after every `every`-th optimise once a key-frame outside the window exists.  Every re-link is held to the model and recorded as
    a CASE (the inputs of the device calls and what they must leave) -> (cases, counters)"""
    seed, window, n_kf, n_steps, extras = spec
    m = rm.RelinkMap(chain, window)
    rng = np.random.default_rng([int(seed), 0x51C])
    feats, cases, seen = {}, [], {k: 0 for k in COUNTERS}
    n_opt, frame = 0, 0
    for ev in wm.history(seed, m, K, n_kf, n_steps, tuple(e for e in extras if e != "capacity")):
        if ev.kind == "correct":
            m.correct(ev.rigid, ev.moves)
            continue
        if ev.kind in ("insert", "refused"):
            rep = m.insert_keyframe(ev.ins)
            if ev.kind == "insert":
                assert rep["status"] == wm.OK
                feats[ev.ins.kf_id] = list(ev.ins.feats)
                frame += 3
            continue
        assert ev.kind == "optimize"
        m.optimize(ev.flags, lambda: {k: kf.pose for k, kf in m.active_kfs.items()}, lambda: {i: mp.pos for i, mp in m.active_mps.items()})
        n_opt += 1
        old = [k for k in sorted(m.all_kfs) if k not in m.active_kfs and m.links(k)]
        cur_kf = m.cur_kf.id
        if ev.meta.get("idle") or not old or n_opt % every or not feats.get(cur_kf):
            continue
        # ---- one loop: the current key-frame against an old one ----
        loop_kf = old[int(rng.integers(len(old)))]
        mp_ids, state, pos = archive_of(m)
        cur = table_of(m, mp_ids, cur_kf, feats[cur_kf], stale=False)       # the pending table: feature_slots + link upkeep leave no erased slot
        loop = table_of(m, mp_ids, loop_kf, feats[loop_kf])
        made = make_pairs(rng, m, cur_kf, feats[cur_kf], loop_kf, feats[loop_kf])
        pairs = np.full((OUT_CAP, 2), -7, np.int32)
        pairs[:len(made)] = made
        outlier = np.zeros(OUT_CAP, np.uint8)
        outlier[:len(made)] = rng.random(len(made)) < 0.15
        outlier[len(made):] = 1 - (np.arange(OUT_CAP - len(made)) % 2)      # beyond the count: never read
        cstat = int(rng.choice([CORRECT_DONE, CORRECT_DONE, CORRECT_FUSED_ONLY, CORRECT_NOT_NEEDED, CORRECT_SKIPPED]))
        p = plan(pairs, len(made), outlier, cstat, cur, loop, cur_kf, state, len(state), point_cap=len(state) + 5)
        trk = tracker_of(m, cur_kf, feats[cur_kf], frame, 0)
        new_ids = {int(mp_ids[s]) for _, _, s in p["links"] if s >= 0} - set(trk["lm_id"].tolist())
        lm_cap = len(trk["lm_id"]) + len(new_ids) + lm_slack
        trk_in = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in trk.items()}
        case = dict(spec=spec, cur_kf=cur_kf, loop_kf=loop_kf, pairs=pairs, count=len(made), outlier=outlier, correct_status=cstat, cur=cur, loop=loop,
                    mp_id=mp_ids, mp_state=state, mp_pos=pos, plan=p, trk_in=trk_in, lm_cap=lm_cap)
        if p["status"] == SKIPPED:
            seen["skipped_or_not_needed"] += 1
            assert not p["merge"] and not p["adopt"] and not p["links"] and np.array_equal(p["cur"], cur)
        else:
            walked = [tuple(int(v) for v in pairs[i]) for i in range(len(made)) if not outlier[i]]
            seen["outlier_pairs"] += len(made) - len(walked)
            active_before = set(m.active_mps)
            rep = m.relink(walked, cur_kf, loop_kf)
            at = {int(v): i for i, v in enumerate(mp_ids)}
            # the plan is the model's walk
            assert [(int(mp_ids[a]), int(mp_ids[b])) for a, b in p["merge"]] == rep["merges"], (spec, cur_kf)
            assert [(f, int(mp_ids[s])) for f, s in p["adopt"]] == rep["adopts"], (spec, cur_kf)
            assert p["report"][:4] == [len(walked), len(rep["merges"]), len(rep["adopts"]), rep["same"]] and p["report"][4] <= rep["null_loop"]
            # every moved observation ends on the point `target` names for the point it was on
            final = {}
            for kf_id, tag, to in rep["moved"]:
                final[(kf_id, tag)] = to
            for (kf_id, tag), to in final.items():
                assert m.link(kf_id, tag) is m.all_mps[to], (spec, kf_id, tag)
            for a, b in p["merge"]:
                assert p["target"][a] == p["target"][b] and p["target"][a] != a and state[p["target"][a]] != 2
            for s in range(len(state)):
                t = int(p["target"][s])
                assert t == -1 or (p["target"][t] == t and int(mp_ids[t]) in m.all_mps)
            # states
            st, state2 = map_relink(state, p["merge"], len(p["merge"]), OUT_CAP, p["status"])
            assert st == MAP_UPDATED and np.array_equal(state2, archive_of(m)[1]), (spec, cur_kf)
            # the current key-frame's table, through lock()
            want = table_of(m, mp_ids, cur_kf, feats[cur_kf], stale=False)
            got = np.array([-1 if lock(int(e), state2) is None else e for e in p["cur"]], np.int32)
            assert np.array_equal(got, want), (spec, cur_kf, np.nonzero(got != want)[0][:5])
            # a stored copy of the table brought up to date by the link list is the table the plan left
            store = Store(FEAT_CAP)
            store.put(cur_kf, cur, FEAT_CAP)
            assert store.set_links(p["links"]) == len(p["links"]) and np.array_equal(store.gather(cur_kf), p["cur"])
            assert [f for _, f, _ in p["links"]] == sorted({f for _, f, _ in p["links"]})          # feature order, each once
            case["state_after"] = state2
            # the tracker names what the model's features name
            status, hits, opened, shared = tracker_relink(trk, p["links"], mp_ids, pos, state2, lm_cap)
            assert status == OK and hits == len(p["links"])
            links = m.links(cur_kf)
            relinked = {f for _, f, s in p["links"] if s >= 0}
            for _, _, _, tag, _ in feats[cur_kf]:
                L = int(trk["lm"][tag])
                assert (L >= 0) == (tag in links), (spec, cur_kf, tag)
                if L >= 0:
                    mp = links[tag]
                    assert int(trk["lm_id"][L]) == mp.id and np.array_equal(trk["lm_pos"][L], mp.pos), (spec, cur_kf, tag)
                    assert tag not in relinked or bool(trk["lm_outl"][L]) == (mp.id in m.outlier_mps)
            seen["tracker_new_slot"] += opened
            seen["tracker_shared_slot"] += shared
            for a, b in rep["merges"]:
                seen["merge_target_inside_table" if b in active_before else "merge_target_outside_table"] += 1
            froms = [a for a, _ in p["merge"]]
            seen["chain_merge"] += sum(1 for _, b in p["merge"] if b in froms)
            seen["adopt"] += len(rep["adopts"]); seen["same_point"] += rep["same"]; seen["dead_loop_point"] += p["report"][4]
            seen["adopted_then_merged_away"] += sum(1 for _, f, s in p["links"] if s < 0)
            seen["links"] += len(p["links"])
        case["trk_out"] = trk
        cases.append(case)
    return cases, seen


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the rows: myslam_relink_stage_batch, myslam_relink_backend_batch, the AFTER_RELINK mode of the two updates, myslam_relink_first_kf_batch

import backend_ref as br  # noqa: E402
import obs_archive_ref as oa  # noqa: E402

AFTER_RELINK = 2                                    # MYSLAM_MAP_AFTER_RELINK


def stage(st, a, merge, target, plan_status, be_obs_cap=1 << 30, stage_cap=1 << 30):
    """myslam_relink_stage_batch for one item: reads the observation archive `st` (oa.Store) and the map archive `a` BEFORE the merged points are
    erased, changes nothing.  -> dict(status, rows: [(mnKFId, u, v, tag, flags, root id, place in the root's list, final slot)] in move order (the own
    rows of every merged point, merge by merge), merges: [(from id, root id, rows)]).  The final GetObservations() of a point that stands is its own
    rows, then for every merge into it, in order, the whole list the merged point had by then: a merged point's own rows stand at a fixed place."""
    none = lambda s: dict(status=s, rows=[], merges=[])
    if st.err:
        return none(st.err)
    if plan_status != DONE:
        return none(SKIPPED)
    ids, state = a.mp_id, a.mp_state
    if any(not (0 <= x < len(ids) and 0 <= y < len(ids)) or x == y or state[x] == 2 or state[y] == 2 for x, y in merge):
        return none(INVALID)
    tpos = {mid: p for p, mid in enumerate(st.t_id)}
    pool = st.pools[st.pcur]

    def own(s):
        mid = ids[s]
        if mid in tpos:
            return list(st.t_rows[tpos[mid]])
        o, c = st.seg.get(mid, (0, 0))
        return [pool[o + j] for j in range(c)]

    size, rel = {}, []
    for x, y in merge:
        for s in (x, y):
            size.setdefault(s, len(own(s)))
        rel.append(size[y]); size[y] += size[x]
    at = {}
    for i in range(len(merge) - 1, -1, -1):
        x, y = merge[i]
        at[x] = rel[i] + at.get(y, 0)
    rows, merges = [], []
    for x, _ in merge:
        root = int(target[x])
        if not (0 <= root < len(ids)) or int(target[root]) != root or root in at or state[root] == 2:
            return none(INVALID)
        mine = own(x)
        merges.append((ids[x], ids[root], len(mine)))
        rows += [tuple(r) + (ids[root], at[x] + j, root) for j, r in enumerate(mine)]
    froms = {ids[x] for x, _ in merge}
    n_table = sum(len(rs) for rs in st.t_rows) - sum(n for f, _, n in merges if f in tpos) + sum(1 for r in rows if r[5] in tpos)
    live_out = sum(c for mid, (o, c) in st.seg.items() if c > 0 and mid not in tpos and mid not in froms and state[ids.index(mid)] != 2)
    if len(rows) > stage_cap or n_table > be_obs_cap or live_out + sum(1 for r in rows if r[5] not in tpos) > st.row_cap:
        return none(CAPACITY)
    return dict(status=DONE, rows=rows, merges=merges)


def backend_relink(w, stg, obs_cap=1 << 30):
    """myslam_relink_backend_batch on a backend_ref.Map: the merged points leave with all their rows, a target that is in the table gets the moved rows
    at the end of its segment, not active (src/loopclosing.cpp:521-525 is AddObservation alone).  -> dict(status, mp_new_row by INPUT row)"""
    before = sorted(w.mps)
    if stg["status"] != DONE:
        return dict(status=stg["status"], mp_new_row=np.full(len(before), -1, np.int32))
    froms = {f for f, _, _ in stg["merges"]}
    add = {}
    for r in sorted(stg["rows"], key=lambda r: r[6]):
        if r[5] in w.mps and r[5] not in froms:
            add.setdefault(r[5], []).append(r)
    n_new = sum(len(mp.obs) for i, mp in w.mps.items() if i not in froms) + sum(len(v) for v in add.values())
    if n_new > obs_cap:
        return dict(status=CAPACITY, mp_new_row=np.full(len(before), -1, np.int32))
    for mid, rs in add.items():
        mp = w.mps[mid]
        for kf, u, v, tag, fl, _, place, _ in rs:
            assert place == len(mp.obs)
            mp.obs.append(br.Obs(kf, u, v, bool(fl & br.OUTLIER), tag))
    for f in froms:
        w.mps.pop(f, None)
    after = sorted(w.mps)
    return dict(status=OK, mp_new_row=np.array([after.index(i) if i in w.mps else -1 for i in before], np.int32))


def obs_update_relink(st, t, be_status, map_status, a, stg):
    """myslam_obs_archive_update_batch(MYSLAM_MAP_AFTER_RELINK) for one item, after the map's update of the same call: the mirror follows the table
    (the appended rows take their observers' ids from the staged rows), a target outside the table gets its list written afresh (stored rows, then
    the moved ones) by update rule 6, the merged points' segments are dead (their state is 2 by now)"""
    if st.err:
        return st.err
    if be_status != 0 or map_status == oa.SKIPPED:
        return oa.SKIPPED
    state = dict(zip(a.mp_id, a.mp_state))
    now = [int(i) for i in t["mp_id"]]
    segs = oa._segments(t)
    prev = {mid: p for p, mid in enumerate(st.t_id)}
    pool = st.pools[st.pcur]
    add = {}
    for r in sorted(stg["rows"], key=lambda r: r[6]):
        add.setdefault(r[5], []).append(r)
    bad = map_status != oa.UPDATED or stg["status"] != DONE
    bad = bad or any(mid not in prev or mid not in state or len(segs[m]) != len(st.t_rows[prev[mid]]) + len(add.get(mid, [])) for m, mid in enumerate(now))
    bad = bad or any(state.get(mid, 0) != 2 for mid in st.t_id if mid not in now)
    bad = bad or any(state.get(mid, 2) == 2 for mid in add)
    if bad:
        st.err = oa.INVALID
        return oa.INVALID
    stored = lambda mid: [pool[st.seg[mid][0] + j] for j in range(st.seg[mid][1])] if mid in st.seg else []
    fresh = [(mid, stored(mid) + [r[:5] for r in rs]) for mid, rs in sorted(add.items()) if mid not in now]
    rewritten = {mid for mid, _ in fresh}
    keep = sum(c for mid, (o, c) in st.seg.items() if c > 0 and state.get(mid, 2) != 2 and mid not in now and mid not in rewritten)
    n_new = sum(len(rs) for _, rs in fresh)
    if keep + n_new > st.row_cap:
        st.err = oa.CAPACITY
        return oa.CAPACITY
    t_rows = []
    for m, mid in enumerate(now):
        old = st.t_rows[prev[mid]]
        kfs = [r[0] for r in old] + [r[0] for r in add.get(mid, [])]
        t_rows.append([(kfs[j],) + r[1:] for j, r in enumerate(segs[m])])
    if st.used + n_new > st.row_cap:
        dst, base = {}, 0
        for mid, (o, c) in sorted(st.seg.items()):
            if c > 0 and state.get(mid, 2) != 2 and mid not in rewritten:
                for j in range(c):
                    dst[base + j] = pool[o + j]
                st.seg[mid] = (base, c); base += c
        st.pcur ^= 1
        st.pools[st.pcur] = pool = dst
        st.used = base
        st.n_reclaim += 1
    for mid, rs in fresh:
        for j, r in enumerate(rs):
            pool[st.used + j] = tuple(r)
        st.seg[mid] = (st.used, len(rs)); st.used += len(rs)
    st.t_id, st.t_rows = now, t_rows
    return oa.UPDATED


def first_kf(st, a):
    """myslam_relink_first_kf_batch: per archive slot the archive row of GetObservations().front()'s key-frame IN LIST ORDER (the mirror for a point of
    the table, the stored segment else), -1 without a row and for an erased point"""
    tpos = {mid: p for p, mid in enumerate(st.t_id)}
    kf_at = {v: i for i, v in enumerate(a.kf_id)}
    pool = st.pools[st.pcur]
    out = np.full(len(a.mp_id), -1, np.int32)
    for s, mid in enumerate(a.mp_id):
        if a.mp_state[s] == 2:
            continue
        if mid in tpos:
            rows = st.t_rows[tpos[mid]]
            kf = rows[0][0] if rows else None
        else:
            o, c = st.seg.get(mid, (0, 0))
            kf = pool[o][0] if c > 0 else None
        out[s] = kf_at.get(kf, -1) if kf is not None else -1
    return out


def moved_links(stg):
    """the link list of the moved rows: (observer's mnKFId, tag, final slot)"""
    return [(int(r[0]), int(r[3]), int(r[7])) for r in stg["rows"]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# whole histories: the model beside the walks of the back end's tables (w), the map archive (a), the observation archive (st) and the loop store

import map_archive_ref as mr  # noqa: E402
import map_insert_ref as mi  # noqa: E402

ROW_COUNTERS = ("merge_target_outside_table", "merge_target_inside_table", "adopt", "same_point", "chain_merge", "dead_loop_point", "skipped_or_not_needed",
                "out_of_order_front_cull", "returning_fixed_landmark", "reclaim", "moved_rows", "moved_rows_from_store", "links_of_other_key_frames")


def flag_solve(w, flags):
    """a solve that moves nothing and removes exactly the edges whose tags are given (the histories construct them; after a re-link the window is not
    the one they were balanced for, and what the walks are held to here is structure)"""
    _, edge_objs, _ = br.flatten(w)
    out = np.array([o.tag in flags for _, o in edge_objs], np.uint8)
    return lambda poses, pts, ep, el, eo, fixed: (poses, pts, np.where(out, 99.0, 0.5), out, 1, int(out.sum()))


def stored_rows_differ(st, a, m):
    want = {mid: mp.obs for mid, mp in m.all_mps.items() if mid not in m.active_mps}
    got = dict(st.live(a))
    if sorted(got) != sorted(i for i in want if want[i]):
        return "stored ids %s, the model's %s" % (sorted(got)[:8], sorted(want)[:8])
    for mid, rows in got.items():
        kw = [(int(o.kf), np.float32(o.u).tobytes(), np.float32(o.v).tobytes(), int(o.tag), br.OUTLIER if o.outlier else 0) for o in want[mid]]
        kg = [(r[0], np.float32(r[1]).tobytes(), np.float32(r[2]).tobytes(), r[3], r[4]) for r in rows]
        if kw != kg:
            return "rows of map point %d" % mid
    return None


def replay_rows(chain, spec, K, row_cap=1 << 20, every=2, relinks=True, record=False):
    """-> dict(seen, cases, most_live, capacity_at, st).  Every event is applied to the model and to the walks; after every event the back end's tables,
    the stored segments, the states, first_kf (list order), the next flatten (first_active, fixed flags: in the tables) and every stored key-frame's
    feature table must be the model's.  A re-link follows every `every`-th optimise once a key-frame outside the window holds a linked feature."""
    seed, window, n_kf, n_steps, extras = spec
    m = rm.RelinkMap(chain, window)
    w, a, st = br.Map(), mr.Archive(), oa.Store(row_cap)
    store = Store(FEAT_CAP)
    rng = np.random.default_rng([int(seed), 0x51C])
    feats, cases, seen = {}, [], {k: 0 for k in ROW_COUNTERS}
    out = dict(seen=seen, cases=cases, most_live=0, capacity_at=None, st=st, checks=0, first_kf_equals_loop_inputs=True)
    touched, n_opt = set(), 0

    def check(where):
        out["checks"] += 1
        t = br.pack(w)
        why = next((k for k in br.TABLES if np.asarray(t[k]).tobytes() != np.asarray(br.pack(m.active_map())[k]).tobytes()), None)
        why = why or stored_rows_differ(st, a, m)
        ids, state, _ = archive_of(m)
        if why is None and (list(ids) != list(a.mp_id) or not np.array_equal(state, np.array(a.mp_state, np.uint8))):
            why = "states"
        if why is None:
            kfs = sorted(m.all_kfs)
            want = [kfs.index(m.all_mps[i].obs[0].kf) if (i in m.all_mps and m.all_mps[i].obs) else -1 for i in a.mp_id]
            got = first_kf(st, a)
            if got.tolist() != want:
                why = "first_kf"
            old = mr.loop_inputs(a, t, m.cur_kf.id, m.cur_kf.id, 0)["first_kf"]
            if not touched:                                                 # no re-link so far: the minimum rule is exact and must agree
                out["first_kf_equals_loop_inputs"] &= old.tolist() == want
            for s, i in enumerate(a.mp_id):                                 # where the two rules differ the list order is the model's
                if i in touched and want[s] != old[s] and want[s] >= 0:
                    seen["out_of_order_front_cull"] += 1
        if why is None:
            for kf_id in store.ids:
                row = lu.filter_landmarks(store.gather(kf_id), a.mp_state)[0]
                links = m.links(kf_id)
                at = {int(v): i for i, v in enumerate(a.mp_id)}
                want_row = np.full(FEAT_CAP, -1, np.int32)
                for _, _, _, tag, _ in feats[kf_id]:
                    if tag in links:
                        want_row[tag] = at[links[tag].id]
                if not np.array_equal(row, want_row):
                    why = "stored table of key-frame %d at %s" % (kf_id, np.nonzero(row != want_row)[0][:4])
                    break
        out["most_live"] = max(out["most_live"], sum(len(rs) for _, rs in st.live(a)))
        assert why is None, (spec, where, why)

    n_ev = -1
    for ev in wm.history(seed, m, K, n_kf, n_steps, tuple(e for e in extras if e != "capacity")):
        n_ev += 1
        if ev.kind == "correct":
            m.correct(ev.rigid, ev.moves)
            for k in w.kfs:
                w.kfs[k] = m.all_kfs[k].pose.copy()
            for i, mp in w.mps.items():
                mp.pos = m.all_mps[i].pos.copy()
            continue
        if ev.kind in ("insert", "refused"):
            ins = ev.ins
            ps, priors = oa.prior_rows(st, [f[0] for f in ins.feats], sorted(w.mps), a)
            assert ps == oa.OK and oa.same_priors(priors, m.priors_for(ins.feats)), (spec, ins.kf_id)
            seen["returning_fixed_landmark"] += len({p[0] for p in priors} & touched)
            rmod = m.insert_keyframe(ins)
            ins.priors = priors
            rw = mi.insert_walk(w, ins, window, 0.2, lambda pk, pn, row: m.dist(pk, pn))
            assert rw["status"] == rmod["status"] == (mi.INVALID if ev.kind == "refused" else mi.OK)
            ms = mr.update(chain, a, mr.AFTER_INSERT, br.pack(w), rw["status"], outlier_ids=ins.outlier_ids)
            so = oa.update(st, oa.AFTER_INSERT, br.pack(w), rw["status"], ms, a)
            if so == oa.CAPACITY:
                out["capacity_at"] = (n_ev, "insert"); return out
            if ev.kind == "insert":
                feats[ins.kf_id] = list(ins.feats)
                ids, n_feat = lu.feat_ids_by_tag(ins.feats)
                table = np.concatenate([mr.feature_slots(a, ids[:n_feat]), np.full(FEAT_CAP - n_feat, -1, np.int32)])
                store.put(ins.kf_id, table, FEAT_CAP)
                if record and cases and cases[-1]["next_insert"] is None:
                    cases[-1]["next_insert"] = ins                           # the key-frame that follows the re-link: returning points come through prior_rows
                check("insert of key-frame %d" % ins.kf_id)
            continue
        assert ev.kind == "optimize"
        t_in = br.pack(w)
        rmod = m.optimize(ev.flags, lambda: {k: kf.pose for k, kf in m.active_kfs.items()}, lambda: {i: mp.pos for i, mp in m.active_mps.items()})
        rw = br.walk(w, flag_solve(w, ev.flags))
        assert rw["status"] == rmod["status"]
        if rw["status"] == br.DONE:
            assert np.array_equal(rw["obs_report"], rmod["obs_report"])
            store.clear_links(lu.culled_list(t_in, rw["obs_report"]))
        ms = mr.update(chain, a, mr.AFTER_OPTIMIZE, br.pack(w), rw["status"], mp_report=rw["mp_report"], left_pos=rw["left_pos"])
        so = oa.update(st, oa.AFTER_OPTIMIZE, br.pack(w), rw["status"], ms, a, obs_report=rw["obs_report"])
        if so == oa.CAPACITY:
            out["capacity_at"] = (n_ev, "optimize"); return out
        check("optimise after key-frame %d" % max(m.all_kfs))
        n_opt += 1
        old = [k for k in sorted(m.all_kfs) if k not in m.active_kfs and m.links(k)]
        cur_kf = m.cur_kf.id
        if not relinks or ev.meta.get("idle") or not old or n_opt % every or not feats.get(cur_kf) or cur_kf not in m.active_kfs:
            continue
        # ---- one loop: the current key-frame against an old one ----
        loop_kf = old[int(rng.integers(len(old)))]
        state = np.array(a.mp_state, np.uint8)
        cur = lu.filter_landmarks(store.gather(cur_kf), state)[0]
        loop = store.gather(loop_kf)                                        # stale links and all; the plan reads lock()
        made = make_pairs(rng, m, cur_kf, feats[cur_kf], loop_kf, feats[loop_kf])
        pairs = np.full((OUT_CAP, 2), -7, np.int32); pairs[:len(made)] = made
        outlier = np.zeros(OUT_CAP, np.uint8); outlier[:len(made)] = rng.random(len(made)) < 0.15
        cstat = int(rng.choice([CORRECT_DONE, CORRECT_DONE, CORRECT_DONE, CORRECT_FUSED_ONLY, CORRECT_NOT_NEEDED, CORRECT_SKIPPED]))
        p = plan(pairs, len(made), outlier, cstat, cur, loop, cur_kf, state, len(state))
        stg = stage(st, a, p["merge"], p["target"], p["status"])
        case = dict(spec=spec, after_event=n_ev, cur_kf=cur_kf, loop_kf=loop_kf, pairs=pairs, count=len(made), outlier=outlier, correct_status=cstat, cur=cur,
                    loop=loop, plan=p, stage=stg, next_insert=None)
        if record:
            import copy
            case.update(w_before=w.clone(), a_before=copy.deepcopy(a), st_before=st.clone(), window=window)
        if stg["status"] == CAPACITY:
            out["capacity_at"] = (n_ev, "relink"); return out
        active_before = set(m.active_mps)
        be = backend_relink(w, stg)
        mst, state2 = map_relink(state, p["merge"], len(p["merge"]), OUT_CAP, be["status"])
        a.mp_state = [int(v) for v in state2]
        ms = mr.update(chain, a, mr.AFTER_INSERT, br.pack(w), be["status"])
        n_rec = st.n_reclaim
        so = obs_update_relink(st, br.pack(w), be["status"], ms, a, stg)
        if so == oa.CAPACITY:
            out["capacity_at"] = (n_ev, "relink"); return out
        seen["reclaim"] += st.n_reclaim - n_rec
        if p["status"] != DONE:
            seen["skipped_or_not_needed"] += 1
            assert be["status"] == SKIPPED and mst == MAP_SKIPPED and ms == mr.SKIPPED and so == oa.SKIPPED
        else:
            assert be["status"] == OK and mst == MAP_UPDATED and ms == mr.UPDATED and so == oa.UPDATED, (spec, be["status"], mst, ms, so)
            walked = [tuple(int(v) for v in pairs[i]) for i in range(len(made)) if not outlier[i]]
            rep = m.relink(walked, cur_kf, loop_kf)
            assert [(int(a.mp_id[x]), int(a.mp_id[y])) for x, y in p["merge"]] == rep["merges"], (spec, cur_kf)
            assert [(f, int(a.mp_id[s])) for f, s in p["adopt"]] == rep["adopts"]
            links = moved_links(stg)
            in_table = {i for i in st.t_id}
            hits = store.set_links(links) + store.set_links(p["links"])
            touched |= {int(a.mp_id[int(p["target"][x])]) for x, _ in p["merge"]}
            for x, y in rep["merges"]:
                seen["merge_target_inside_table" if y in active_before else "merge_target_outside_table"] += 1
            froms = [x for x, _ in p["merge"]]
            seen["chain_merge"] += sum(1 for _, y in p["merge"] if y in froms)
            seen["adopt"] += len(rep["adopts"]); seen["same_point"] += rep["same"]; seen["dead_loop_point"] += p["report"][4]
            seen["moved_rows"] += len(stg["rows"]); seen["moved_rows_from_store"] += sum(n for f, _, n in stg["merges"] if f not in active_before)
            seen["links_of_other_key_frames"] += sum(1 for k, _, _ in links if k != cur_kf and k in store.ids)
            assert hits >= len(p["links"])
        case["touched"] = set(touched)
        cases.append(case)
        check("re-link at key-frame %d" % cur_kf)
    return out
