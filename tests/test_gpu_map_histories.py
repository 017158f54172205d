"""The device's map tables through whole random histories (tests/whole_map_model.py), held against the object model of the reference's Map: batches of
6 histories run as 6 items of one api.Backend + api.MapArchive pair on one stream.  After each call of a key-frame (insert, update, optimise, update)
everything is read back: the back end's tables must be backend_ref.pack of the model's active part byte for byte, the reports the walks', d_obs_report == 1
exactly the constructed outlier edges, the archive map_archive_ref's walk byte for byte (internals included) and check_against_chain's against the model.
The model takes its numbers after an optimise from the device (the tables' poses, the solve's positions); its structure never.

`window` is an argument of the insert call, not of an item: a batch whose histories have two windows takes two insert calls per key-frame, and in
each the items of the other window are handed a key-frame the call refuses (a feature id below -1), so refused and skipped items sit next to running
ones in every call; so do finished ones (tests/whole_map_model.history goes on with refused inserts and idle optimises) and the item that meets the
archive's caps exactly on its last key-frame and is refused with MYSLAM_ERR_CAPACITY on the next."""
import hashlib

import numpy as np
import pytest

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
import test_whole_map_model as T
import whole_map_model as wm
from test_gpu_map_archive import Dev, tables_of
from test_gpu_map_insert import OUT_FILL, TABLE_ARGS, Run, check_item

pytestmark = pytest.mark.gpu

BATCHES = (T.HISTORIES[:6], T.HISTORIES[6:])
FEAT_CAP, PRIOR_CAP, OUTLIER_CAP = 128, 96, 64
BE_CAPS = (8, 96, 1536)
PARKED = mi.Insert(1, mi.IDENT, [(-2, (0.0, 0.0, 0.0), (1.0, 2.0), 7, False)])        # a feature id below -1: refused whatever the table holds
OPT_OUT = ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2", "rounds", "n_out", "status")
LOAD = ("kf_id", "kf_pose", "edge_v0", "edge_v1", "meas", "mp_id", "mp_pos", "mp_first_kf", "mp_state", "snapshot", "mp_gone_kf", "mp_win_mask", "win_kf")


class Item:
    def __init__(self, pkg, spec):
        self.spec = spec
        self.m = wm.WholeMap(pkg.chain, spec[1]) if spec else None
        self.gen = wm.history(spec[0], self.m, T.K, spec[2], spec[3], spec[4]) if spec else iter(())
        self.w, self.a = br.Map(), mr.Archive()
        self.window = spec[1] if spec else None
        self.sha = hashlib.sha1()
        self.rng = np.random.default_rng([spec[0], 0x99]) if spec else None
        self.seen = dict(capacity=0, refused=0, empty=0, corrected=0, outliers=0)

    def digest(self, *arrays):
        for x in arrays:
            self.sha.update(np.ascontiguousarray(x).tobytes())


def run_batch(api, pkg, specs, arch_caps):
    """-> the items, after every history has run to its end"""
    import torch
    chain = pkg.chain
    B = len(specs)
    items = [Item(pkg, s) for s in specs]
    windows = sorted({it.window for it in items if it.spec})
    r = Run(api, [br.Map() for _ in range(B)], [PARKED] * B, windows[0], 0.2, caps=(BE_CAPS, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP))
    dev = Dev(api, B, arch_caps, BE_CAPS, r.stream)
    dev.h.attach_solve(*r.h.solve_view())                                   # a point that leaves with an optimise takes the solve's position
    full = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    oo = dict(obs_report=full((B, BE_CAPS[2]), torch.uint8), mp_report=full((B, BE_CAPS[1]), torch.uint8), new_outlier=full((B, BE_CAPS[1]), torch.int32),
              n_new=full((B,), torch.int32), obs_chi2=full((B, BE_CAPS[2]), torch.float64), rounds=full((B,), torch.int32), n_out=full((B,), torch.int32),
              status=full((B,), torch.int32))
    r.stream.wait_stream(torch.cuda.current_stream())
    p = lambda t: t.data_ptr()
    host = {k: v.copy() for k, v in r.host.items()}

    def read_tables():
        r.stream.synchronize()
        return {k: v.cpu().numpy() for k, v in r.d.items()}

    def check_state(it, b, host, where):
        """the tables are the model's active part; the archive is the walk's and the model's"""
        t, want = tables_of(host, b), br.pack(it.m.active_map())
        for k in br.TABLES:
            n = len(want[k])
            assert host[k][b, :n].tobytes() == want[k].tobytes() and host[k].dtype == want[k].dtype, (it.spec, where, k)
        assert (host["n_kf"][b], host["n_mp"][b], host["n_obs"][b]) == (len(want["kf_id"]), len(want["mp_id"]), len(want["obs_mp"])), (it.spec, where)
        got = dev.h.get(b)
        assert mr.same(got, it.a.arrays()) is None, (it.spec, where, mr.same(got, it.a.arrays()))
        why = mr.check_against_chain(it.a, it.m, it.m.erased)
        assert why is None, (it.spec, where, why)
        it.digest(*[t[k] for k in ("kf_id", "kf_pose", "mp_id", "mp_pos", "obs_mp", "obs_kf", "obs_flags")], *[got[k] for k in mr.FIELDS])

    step = 0
    while True:
        # ---- the next event of every item; corrections first (the archive is overwritten with moved values, write_backend carries them to the tables)
        evs, corrected = [], []
        for b, it in enumerate(items):
            ev = next(it.gen, None)
            while ev is not None and ev.kind == "correct":
                it.m.correct(ev.rigid, ev.moves)
                if b not in corrected:
                    corrected.append(b)
                ev = next(it.gen, None)
            evs.append(ev)
        if all(ev is None for ev in evs):
            break
        if corrected:
            sel = np.zeros(B, np.uint8); sel[corrected] = 1
            for b in corrected:
                it = items[b]
                arch = dev.h.get(b)
                for row, kid in enumerate(it.a.kf_id):
                    arch["kf_pose"][row] = it.a.kf_pose[row] = it.m.all_kfs[kid].pose.copy()
                for s, mid in enumerate(it.a.mp_id):
                    if mid in it.m.all_mps:
                        arch["mp_pos"][s] = it.a.mp_pos[s] = it.m.all_mps[mid].pos.copy()
                dev.h.load(b, *[arch[k] for k in LOAD])
                for kid in it.w.kfs:
                    it.w.kfs[kid] = it.m.all_kfs[kid].pose.copy()
                for mid, mp in it.w.mps.items():
                    mp.pos = it.m.all_mps[mid].pos.copy()
                it.seen["corrected"] += 1
            d_sel = torch.from_numpy(sel).cuda()
            r.stream.wait_stream(torch.cuda.current_stream())
            dev.h.write_backend_batch(p(r.d["kf_id"]), p(r.d["kf_pose"]), p(r.d["n_kf"]), BE_CAPS[0], p(r.d["mp_id"]), p(r.d["mp_pos"]), p(r.d["n_mp"]), BE_CAPS[1],
                                      p(d_sel), B)
            after = read_tables()
            for b, it in enumerate(items):
                if b in corrected:                                          # rows found by id; the next update is then a copy of equal bits
                    check_state(it, b, after, "write-back before step %d" % step)
                for k in after:                                             # beyond the counts, and every unselected item: untouched
                    x, y = after[k][b:b + 1], host[k][b:b + 1]
                    if b in corrected and k in ("kf_pose", "mp_pos"):
                        n = int(after["n_kf" if k == "kf_pose" else "n_mp"][b])
                        x, y = x[:, n:], y[:, n:]
                    assert x.tobytes() == y.tobytes(), (b, k)
            host = after
        # ---- the inserts: one call per window, the items of the other windows parked
        for W in windows:
            inss = []
            for it, ev in zip(items, evs):
                live = ev is not None and it.window == W
                if live:
                    ev.ins.priors = it.m.priors_for(ev.ins.feats)
                inss.append(ev.ins if live else PARKED)
            r.inp = mi.pack_inputs(inss, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP)
            with torch.cuda.stream(r.stream):
                for k, v in r.inp.items():
                    r.di[k].copy_(torch.from_numpy(v))
                for k, v in r.o.items():
                    v.fill_(OUT_FILL[k])
            r.enqueue(window=W)
            dev.update(mr.AFTER_INSERT, r.d, r.o["status"], r.di["outlier_mp_id"], r.di["n_outlier"], OUTLIER_CAP)
            out = r.results()
            for b, (it, ev) in enumerate(zip(items, evs)):
                live = ev is not None and it.window == W
                w_after, rw = check_item(r, host, out, b, it.w, inss[b], window=W)          # every table and report WHOLE against the walk
                before = it.a.arrays()
                st = mr.update(chain, it.a, mr.AFTER_INSERT, tables_of(out, b), rw["status"], outlier_ids=inss[b].outlier_ids, caps=arch_caps)
                assert dev.status.cpu().numpy()[b] == st, (it.spec, step, st)
                if not live or ev.kind == "refused":
                    assert rw["status"] == mi.INVALID and st == mr.SKIPPED
                    it.seen["refused"] += int(live)
                elif ev.kind == "capacity":                                 # the back end took the key-frame, the archive could not: every byte kept
                    assert rw["status"] == mi.OK and st == mr.CAPACITY and mr.same(dev.h.get(b), before) is None
                    it.seen["capacity"] += 1
                    it.gen = iter(())
                    continue
                else:
                    rm = it.m.insert_keyframe(ev.ins)
                    assert rw["status"] == rm["status"] == mi.OK and st == mr.UPDATED
                    assert rw["removed_kf_id"] == rm["removed_kf_id"] and rw["branch"] == rm["branch"], (it.spec, step)
                    assert not rm["branch"] or wm.margins_ok(rm, 0.2, wm.MARGIN)
                    it.w = w_after
                if it.spec and it.m.all_kfs:
                    check_state(it, b, out, "insert call of window %d, step %d" % (W, step))
                elif not it.spec:
                    assert out["n_kf"][b] == out["n_mp"][b] == out["n_obs"][b] == 0 and len(dev.h.get(b)["kf_id"]) == 0
            host = {k: out[k] for k in host}
        if all(ev is None or ev.kind == "capacity" for ev in evs):
            break
        # ---- the optimise
        opts = [next(it.gen, None) if (ev is not None and ev.kind != "capacity") else None for it, ev in zip(items, evs)]
        assert all(o is None or o.kind == "optimize" for o in opts)
        r.h.optimize_batch(*[p(r.d[k]) for k in TABLE_ARGS], B, T.K, *[p(oo[k]) for k in OPT_OUT])
        dev.update(mr.AFTER_OPTIMIZE, r.d, oo["status"], report=oo["mp_report"])
        after = read_tables()
        rep = {k: v.cpu().numpy() for k, v in oo.items()}
        ast = dev.status.cpu().numpy()
        for b, (it, ev) in enumerate(zip(items, opts)):
            if ev is None:                                                  # an empty item, or the one that ran into the archive's caps
                if not it.spec:
                    assert rep["status"][b] == br.EMPTY and ast[b] == mr.SKIPPED
                continue
            t_in = tables_of(host, b)
            flat = r.h.debug_flat(b)

            def poses(b=b, it=it):
                return {int(k): after["kf_pose"][b, i] for i, k in enumerate(after["kf_id"][b, :int(after["n_kf"][b])])}

            def points(b=b, t_in=t_in, flat=flat):
                x = r.h.debug_solved(b)[1]
                return {int(t_in["mp_id"][row]): x[j] for j, row in enumerate(flat["pt_src"])}

            rm = it.m.optimize(ev.flags, poses, points)
            rw = br.walk(it.w, lambda *a, b=b: r.h.debug_solved(b))
            assert rep["status"][b] == rw["status"] == rm["status"], (it.spec, step)
            n_mp, n_obs = len(t_in["mp_id"]), len(t_in["obs_mp"])
            if rm["status"] == br.DONE:
                # d_obs_report == 1 marks exactly the constructed outlier edges; both reports are the model's and the walk's
                assert np.array_equal(rep["obs_report"][b, :n_obs], rm["obs_report"]) and np.array_equal(rw["obs_report"], rm["obs_report"]), (it.spec, step)
                assert np.array_equal(rep["mp_report"][b, :n_mp], rm["mp_report"]) and np.array_equal(rw["mp_report"], rm["mp_report"]), (it.spec, step)
                assert int((rm["obs_report"] == 1).sum()) == len(ev.flags) == rep["n_out"][b]
                it.seen["outliers"] += len(ev.flags)
            else:
                assert not ev.flags and not rep["obs_report"][b, :n_obs].any() and not rep["mp_report"][b, :n_mp].any()  # the item's rows: as far as its counts reach
                it.seen["empty"] += 1
            st = mr.update(chain, it.a, mr.AFTER_OPTIMIZE, tables_of(after, b), rw["status"], mp_report=rep["mp_report"][b], caps=arch_caps, left_pos=rw["left_pos"])
            assert ast[b] == st == (mr.UPDATED if rm["status"] == br.DONE else mr.SKIPPED), (it.spec, step, ast[b], st)
            check_state(it, b, after, "optimise of step %d" % step)
            it.digest(rep["obs_report"][b, :n_obs], rep["mp_report"][b, :n_mp])
        host = after
        if step % 3 == 2:
            check_loop_inputs(api, items, r, dev, host)
        step += 1
    return items


def check_loop_inputs(api, items, r, dev, host):
    """loop_inputs_batch and feature_slots_batch against the model's own lists: the loop id an older key-frame or an absent one, a candidate or none"""
    import torch
    B = len(items)
    live = [it.spec is not None and bool(it.m.all_kfs) for it in items]
    cur = [it.m.cur_kf.id if ok else -1 for it, ok in zip(items, live)]
    loop, det = [], []
    for it, ok in zip(items, live):
        ids = sorted(it.m.all_kfs) if ok else [0]
        loop.append(ids[int(it.rng.integers(len(ids)))] if (ok and it.rng.random() < 0.7) else 10 ** 6)
        det.append(int(it.rng.random() < 0.3) if ok else 0)
    pc = dev.caps[2]
    full = lambda shape: torch.full(shape, -4321, dtype=torch.int32, device="cuda")
    o = dict(active=full((B, BE_CAPS[0])), n_active=full((B,)), cur=full((B,)), loop=full((B,)), first_active=full((B, pc)), first_kf=full((B, pc)), n_points=full((B,)))
    i = dict(cur=torch.tensor(cur, dtype=torch.int64, device="cuda"), loop=torch.tensor(loop, dtype=torch.int64, device="cuda"),
             det=torch.tensor(det, dtype=torch.int32, device="cuda"))
    feat = np.full((B, FEAT_CAP), -66, np.int64); nf = np.zeros(B, np.int32)
    for b, (it, ok) in enumerate(zip(items, live)):
        if ok:
            ids = (list(it.a.mp_id) + [-1, 10 ** 7, it.a.mp_id[-1] + 1])[-FEAT_CAP:]
            feat[b, :len(ids)] = ids; nf[b] = len(ids)
    d_feat, d_nf = torch.from_numpy(feat).cuda(), torch.from_numpy(nf).cuda()
    slots = full((B, FEAT_CAP))
    r.stream.wait_stream(torch.cuda.current_stream())
    p = lambda t: t.data_ptr()
    d = r.d
    dev.h.loop_inputs_batch(p(d["kf_id"]), p(d["n_kf"]), BE_CAPS[0], p(d["mp_id"]), p(d["n_mp"]), BE_CAPS[1], p(d["obs_mp"]), p(d["obs_kf"]), p(d["obs_flags"]),
                            p(d["n_obs"]), BE_CAPS[2], p(i["cur"]), p(i["loop"]), p(i["det"]), BE_CAPS[0], B,
                            *[p(o[k]) for k in ("active", "n_active", "cur", "loop", "first_active", "first_kf", "n_points")])
    dev.h.feature_slots_batch(p(d_feat), p(d_nf), FEAT_CAP, B, p(slots))
    r.stream.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    gs = slots.cpu().numpy()
    for b, (it, ok) in enumerate(zip(items, live)):
        if not ok:
            assert got["cur"][b] == -1 and got["loop"][b] == -1 and got["n_active"][b] == 0 and got["n_points"][b] == 0
            continue
        want = T.model_loop_inputs(it.m, cur[b], loop[b], det[b], it.a.mp_id)
        n = want["n_points"]
        assert got["n_points"][b] == n and got["n_active"][b] == len(want["active"]) and got["cur"][b] == want["cur"] and got["loop"][b] == want["loop"], it.spec
        assert got["active"][b, :len(want["active"])].tolist() == want["active"], it.spec
        assert got["first_active"][b, :n].tolist() == want["first_active"] and got["first_kf"][b, :n].tolist() == want["first_kf"], it.spec
        assert (got["first_kf"][b, n:] == -4321).all()
        ids = feat[b, :nf[b]]
        assert gs[b, :nf[b]].tolist() == [(it.a.mp_id.index(int(v)) if int(v) in it.m.all_mps else -1) for v in ids], it.spec


def caps_for(pkg, oracle, specs):
    """the archive's caps of a batch: what its history with the capacity extra meets exactly (the model's own CPU run says what that is), which the
    other histories of the batch must stay within"""
    finals = {s: T.caps_of(pkg, oracle, s) for s in specs}
    tight = [s for s in specs if "capacity" in s[4]]
    caps = finals[tight[0]] if tight else tuple(max(f[i] for f in finals.values()) + 2 for i in range(3))
    assert all(f[i] <= caps[i] for f in finals.values() for i in range(3)), (caps, finals)
    return caps


@pytest.mark.parametrize("n", range(len(BATCHES)))
def test_six_histories_side_by_side(api, pkg, oracle, n):
    specs = BATCHES[n]
    assert len(specs) == 6 and len({s[1] for s in specs}) == 2 and len({s[2] for s in specs}) >= 2
    caps = caps_for(pkg, oracle, specs)
    items = run_batch(api, pkg, list(specs), caps)
    seen = {k: sum(it.seen[k] for it in items) for k in items[0].seen}
    print("batch %d:" % n, seen, "archive caps", caps)
    for it in items:
        assert len(it.m.all_kfs) == it.spec[2]
    assert seen["capacity"] == sum("capacity" in s[4] for s in specs) and seen["refused"] >= 1 and seen["outliers"] >= 20
    assert seen["empty"] >= sum("empty" in s[4] for s in specs) and seen["corrected"] >= sum("rigid" in s[4] for s in specs)


def test_items_do_not_depend_on_slot_or_neighbours(api, pkg, oracle):
    """two histories once more, in other slots, in the other order, next to an untouched empty item instead of their neighbours: every byte that was read
    back after every call (tables up to their counts, the whole archive, the reports) must be what it was"""
    two = [BATCHES[0][1], BATCHES[0][3]]                                    # a window of 3 with a correction, a window of 2 with an EMPTY optimise
    assert two[0][1] != two[1][1] and not any("capacity" in s[4] for s in two)
    caps = tuple(v + 4 for v in caps_for(pkg, oracle, two))
    first = run_batch(api, pkg, [two[0], two[1], None], caps)
    second = run_batch(api, pkg, [None, two[1], two[0]], caps)
    assert first[0].sha.hexdigest() == second[2].sha.hexdigest() and first[1].sha.hexdigest() == second[1].sha.hexdigest()
    assert first[0].sha.hexdigest() != first[1].sha.hexdigest()
    for it in (first[2], second[0]):
        assert not it.a.kf_id and not it.w.kfs


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The named case (tests/test_whole_map_model.py holds its CPU form with a made-up solve): a landmark that is NOT fixed loses every active observation to
# the optimiser while a row of a key-frame that left remains.  No balanced history reaches it; here the device's own solve is brought to it.

def leaving_point_case(chain):
    """window 2, pure translations along x.  Key-frame 0 makes twelve exact points; key-frame 1 sees them and makes P = 200; key-frame 2 sees them all
    (key-frame 0, the farthest, leaves: the twelve are fixed from now on and hold the poses in place); key-frame 3 (0.125 from key-frame 2: the nearest
    branch, key-frame 2 leaves) sees them all again.  P's pixels in key-frames 1 and 3 are 8 px above and below its projection (chi2 64 against the threshold 5.991; a larger gap only makes the ten iterations wander): the epipolar lines
    run along u, no position brings the two together, both edges fail, and P keeps the row of key-frame 2 alone.
    -> (model, walk map, archive walk, the tags of P's two active rows)"""
    m, w, a = wm.WholeMap(chain, 2), br.Map(), mr.Archive()
    pts = {100 + i: np.array([-3.0 + 0.5 * i, -1.0 + 0.25 * (i % 5), 8.0 + 0.5 * (i % 4)]) for i in range(12)}
    pts[200] = np.array([0.25, 0.5, 10.0])
    tag, bad = [0], []
    for kf_id, x in ((0, -1.0), (1, 0.0), (2, 1.0), (3, 1.125)):
        pose = mi.shifted(x)
        feats = []
        for mid, pw in sorted(pts.items()):
            if mid == 200 and kf_id == 0:
                continue
            uv, _ = wm.project(chain, T.K, pose, pw)
            dv = {1: 8.0, 3: -8.0}.get(kf_id, 0.0) if mid == 200 else 0.0
            tag[0] += 1
            feats.append((mid, tuple(pw), (np.float32(uv[0]), np.float32(uv[1] + dv)), tag[0], False))
            if dv:
                bad.append(tag[0])
        ins = mi.Insert(kf_id, pose, feats)
        ins.priors = m.priors_for(ins.feats)
        rw = mi.insert_walk(w, ins, 2, 0.2, lambda pk, pn, row: m.dist(pk, pn))
        rm = m.insert_keyframe(ins)
        assert rw["status"] == rm["status"] == mi.OK and mr.update(chain, a, mr.AFTER_INSERT, br.pack(w), 0) == mr.UPDATED
    assert sorted(m.active_kfs) == [1, 3] and [int(o.kf) for o in m.all_mps[200].obs] == [1, 2, 3] and len(m.all_mps[200].active_obs) == 2
    return m, w, a, bad


@pytest.mark.parametrize("attached", [True, False])
def test_named_case_a_moved_point_leaves_the_active_set_alive(api, pkg, attached):
    import torch
    chain = pkg.chain
    m, w, a, bad = leaving_point_case(chain)
    r = Run(api, [w], [PARKED], 2, 0.2, caps=(BE_CAPS, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP))
    dev = Dev(api, 1, (8, 8, 40), BE_CAPS, r.stream)
    arr = a.arrays()
    dev.h.load(0, *[arr[k] for k in LOAD])
    if attached:
        dev.h.attach_solve(*r.h.solve_view())
    full = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    oo = dict(obs_report=full((1, BE_CAPS[2]), torch.uint8), mp_report=full((1, BE_CAPS[1]), torch.uint8), new_outlier=full((1, BE_CAPS[1]), torch.int32),
              n_new=full((1,), torch.int32), obs_chi2=full((1, BE_CAPS[2]), torch.float64), rounds=full((1,), torch.int32), n_out=full((1,), torch.int32),
              status=full((1,), torch.int32))
    r.stream.wait_stream(torch.cuda.current_stream())
    p = lambda t: t.data_ptr()
    t_in = br.pack(w)
    r.h.optimize_batch(*[p(r.d[k]) for k in TABLE_ARGS], 1, T.K, *[p(oo[k]) for k in OPT_OUT])
    dev.update(mr.AFTER_OPTIMIZE, r.d, oo["status"], report=oo["mp_report"])
    r.stream.synchronize()
    after = {k: v.cpu().numpy() for k, v in r.d.items()}
    rep = {k: v.cpu().numpy() for k, v in oo.items()}
    flat, solved = r.h.debug_flat(0), r.h.debug_solved(0)
    rm = m.optimize(set(bad), {int(k): after["kf_pose"][0, i] for i, k in enumerate(after["kf_id"][0, :2])},
                    {int(t_in["mp_id"][row]): solved[1][j] for j, row in enumerate(flat["pt_src"])})
    rw = br.walk(w, lambda *x: solved)
    n_mp, n_obs = len(t_in["mp_id"]), len(t_in["obs_mp"])
    assert rep["status"][0] == br.DONE and rm["left_alive"] == [200] and not flat["fixed"][list(t_in["mp_id"][flat["pt_src"]]).index(200)]
    assert np.array_equal(rep["obs_report"][0, :n_obs], rm["obs_report"]) and np.array_equal(rep["mp_report"][0, :n_mp], rm["mp_report"])      # exactly P's two rows
    assert np.array_equal(rw["mp_report"], rm["mp_report"]) and list(rw["left_pos"]) == [n_mp - 1]
    moved = float(np.abs(m.all_mps[200].pos - np.array([0.25, 0.5, 10.0])).max())
    print("map point 200 moved by", moved)
    assert moved > 1e-6                                                     # the solve did move it: otherwise the case shows nothing
    st = mr.update(chain, a, mr.AFTER_OPTIMIZE, tables_of(after, 0), rw["status"], mp_report=rep["mp_report"][0], left_pos=rw["left_pos"] if attached else None)
    got = dev.h.get(0)
    assert dev.status.cpu().numpy()[0] == st == mr.UPDATED and mr.same(got, a.arrays()) is None, mr.same(got, a.arrays())
    assert mr.check_against_chain(a, m, m.erased) == (None if attached else "position of map point 200")
