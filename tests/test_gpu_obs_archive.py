"""myslam_obs_archive_* (csrc/obs_archive.hip: k_obs_update, k_obs_prior_rows): the observation rows of every map point that is alive and outside the back
end's table, kept on the device, and the prior rows of every insert written from them.  Whole random histories (tests/whole_map_model.py) run as items
of one api.Backend + api.MapArchive + api.ObsArchive on one stream; the prior arrays of every insert are the device pointers prior_rows_batch wrote,
never the model's.  After each call the back end's tables must be backend_ref.pack of the model's active part, api.ObsArchive.get the walk
(tests/obs_archive_ref.py) byte for byte and the model's lists, the prior arrays whole_map_model.priors_for.  Then the reclaim at a history's own
maximum of live rows and one row below it, a hand-made item beyond one pass of the 256-thread workgroup, the edges of the contract, and the gap the
feature closes.  Nothing here is floating point: every comparison is of bytes."""
import hashlib

import numpy as np
import pytest

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
import obs_archive_ref as oa
import test_gpu_map_histories as H
import test_whole_map_model as T
import whole_map_model as wm
from test_gpu_map_archive import Dev, tables_of
from test_gpu_map_insert import OUT_FILL, TABLE_ARGS, Run, check_item
from test_obs_archive_ref import check_against_model

pytestmark = pytest.mark.gpu

FEAT_CAP, PRIOR_CAP, OUTLIER_CAP, BE_CAPS, PARKED, OPT_OUT = H.FEAT_CAP, H.PRIOR_CAP, H.OUTLIER_CAP, H.BE_CAPS, H.PARKED, H.OPT_OUT
PRIOR = ("prior_mp_id", "prior_kf_id", "prior_uv", "prior_tag", "prior_flags")
ROW_CAP = 240                                   # the most live rows of any of the 12 histories is 231
STATUS_FILL = -93


def tables_full(d, b):
    """item b of downloaded back-end tables cut to its counts, pixels and tags included: what the observation archive's walk reads"""
    t = tables_of(d, b)
    no = int(d["n_obs"][b])
    t.update(obs_uv=d["obs_uv"][b, :no], obs_tag=d["obs_tag"][b, :no])
    return t


def priors_of(host, b):
    """item b's prior arrays as the device wrote them, in the form of Insert.priors; the slots from the count on must hold the caller's bytes"""
    n = int(host["n_prior"][b])
    for k in PRIOR:
        rest = host[k][b, n:]
        assert (rest == np.array(mi._FILL[k], rest.dtype)).all(), (b, k)
    return [(int(host["prior_mp_id"][b, i]), int(host["prior_kf_id"][b, i]), tuple(host["prior_uv"][b, i]), int(host["prior_tag"][b, i]),
             bool(host["prior_flags"][b, i] & br.OUTLIER)) for i in range(n)]


class Item:
    def __init__(self, pkg, spec, row_cap):
        self.spec = spec
        self.m = wm.WholeMap(pkg.chain, spec[1]) if spec else None
        self.gen = wm.history(spec[0], self.m, T.K, spec[2], spec[3], spec[4]) if spec else iter(())
        self.w, self.a, self.st = br.Map(), mr.Archive(), oa.Store(row_cap)
        self.window = spec[1] if spec else None
        self.sha = hashlib.sha1()
        self.seen = dict(priors=0, prior_rows=0, stale=0)
        self.capacity_at = None

    def digest(self, *arrays):
        for x in arrays:
            self.sha.update(np.ascontiguousarray(x).tobytes())


class Chain:
    """histories as items of one back end, one map archive and one observation archive; every call is checked when it has run"""

    def __init__(self, api, pkg, specs, arch_caps, row_cap=ROW_CAP, with_obs=True):
        import torch
        self.torch, self.api, self.pkg, self.arch_caps = torch, api, pkg, arch_caps
        self.B = B = len(specs)
        self.items = [Item(pkg, s, row_cap) for s in specs]
        self.windows = sorted({it.window for it in self.items if it.spec})
        self.r = r = Run(api, [br.Map() for _ in range(B)], [PARKED] * B, self.windows[0], 0.2, caps=(BE_CAPS, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP))
        self.dev = Dev(api, B, arch_caps, BE_CAPS, r.stream)
        self.dev.h.attach_solve(*r.h.solve_view())
        self.obs = api.ObsArchive(self.dev.h, B, BE_CAPS[2], row_cap, stream=r.stream.cuda_stream) if with_obs else None
        full = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
        self.oo = dict(obs_report=full((B, BE_CAPS[2]), torch.uint8), mp_report=full((B, BE_CAPS[1]), torch.uint8), new_outlier=full((B, BE_CAPS[1]), torch.int32),
                       n_new=full((B,), torch.int32), obs_chi2=full((B, BE_CAPS[2]), torch.float64), rounds=full((B,), torch.int32),
                       n_out=full((B,), torch.int32), status=full((B,), torch.int32))
        self.ostatus, self.pstatus = full((B,), torch.int32, STATUS_FILL), full((B,), torch.int32, STATUS_FILL)
        r.stream.wait_stream(torch.cuda.current_stream())
        self.host = {k: v.copy() for k, v in r.host.items()}
        self.step = 0

    # ------------------------------------------------------------------------------------------------------------------------- device calls
    def obs_update(self, mode, be_status, report=None):
        p = lambda t: t.data_ptr()
        d = self.r.d
        self.obs.update_batch(mode, *[p(d[k]) for k in TABLE_ARGS], *BE_CAPS, p(be_status), p(self.dev.status), p(report) if report is not None else None,
                              self.B, p(self.ostatus))

    def prior_rows(self):
        p = lambda t: t.data_ptr()
        d, di = self.r.d, self.r.di
        self.obs.prior_rows_batch(p(di["feat_mp_id"]), p(di["n_feat"]), FEAT_CAP, p(d["mp_id"]), p(d["n_mp"]), BE_CAPS[1], self.B,
                                  *[p(di[k]) for k in PRIOR], p(di["n_prior"]), PRIOR_CAP, p(self.pstatus))

    def read_tables(self):
        self.r.stream.synchronize()
        return {k: v.cpu().numpy() for k, v in self.r.d.items()}

    def check_state(self, it, b, host, where):
        want = br.pack(it.m.active_map())
        for k in br.TABLES:
            n = len(want[k])
            assert host[k][b, :n].tobytes() == want[k].tobytes() and host[k].dtype == want[k].dtype, (it.spec, where, k)
        assert (host["n_kf"][b], host["n_mp"][b], host["n_obs"][b]) == (len(want["kf_id"]), len(want["mp_id"]), len(want["obs_mp"])), (it.spec, where)
        if self.obs is None:
            return
        got = self.obs.get(b)
        why = oa.same(got, it.st.arrays(it.a))
        assert why is None, (it.spec, where, why)
        why = check_against_model(it.st, it.a, it.m)
        assert why is None, (it.spec, where, why)
        it.digest(*[got[k] for k in oa.GET_FIELDS])

    # ------------------------------------------------------------------------------------------------------------------------- one key-frame
    def next_events(self):
        """the next event of every item; corrections first, as tests/test_gpu_map_histories.py applies them (pixels do not move: the store is untouched)"""
        torch, r, dev, B = self.torch, self.r, self.dev, self.B
        evs, corrected = [], []
        for b, it in enumerate(self.items):
            ev = next(it.gen, None)
            while ev is not None and ev.kind == "correct":
                it.m.correct(ev.rigid, ev.moves)
                if b not in corrected:
                    corrected.append(b)
                ev = next(it.gen, None)
            evs.append(ev)
        if corrected:
            sel = np.zeros(B, np.uint8); sel[corrected] = 1
            for b in corrected:
                it = self.items[b]
                arch = dev.h.get(b)
                for row, kid in enumerate(it.a.kf_id):
                    arch["kf_pose"][row] = it.a.kf_pose[row] = it.m.all_kfs[kid].pose.copy()
                for s, mid in enumerate(it.a.mp_id):
                    if mid in it.m.all_mps:
                        arch["mp_pos"][s] = it.a.mp_pos[s] = it.m.all_mps[mid].pos.copy()
                dev.h.load(b, *[arch[k] for k in H.LOAD])
                for kid in it.w.kfs:
                    it.w.kfs[kid] = it.m.all_kfs[kid].pose.copy()
                for mid, mp in it.w.mps.items():
                    mp.pos = it.m.all_mps[mid].pos.copy()
            d_sel = torch.from_numpy(sel).cuda()
            r.stream.wait_stream(torch.cuda.current_stream())
            p = lambda t: t.data_ptr()
            dev.h.write_backend_batch(p(r.d["kf_id"]), p(r.d["kf_pose"]), p(r.d["n_kf"]), BE_CAPS[0], p(r.d["mp_id"]), p(r.d["mp_pos"]), p(r.d["n_mp"]), BE_CAPS[1],
                                      p(d_sel), B)
            self.host = self.read_tables()
        self.corrected = bool(corrected)
        return evs

    def insert_call(self, W, evs, null_priors=False):
        """one insert call for the items of window W (the others parked): prior_rows -> insert -> map update -> obs update, then every check.
        -> per item the model's priors of its key-frame (None for items that did not run)"""
        torch, r, dev, chain = self.torch, self.r, self.dev, self.pkg.chain
        items = self.items
        inss, wants = [], []
        for it, ev in zip(items, evs):
            live = ev is not None and it.window == W
            inss.append(ev.ins if live else PARKED)
            wants.append(it.m.priors_for(ev.ins.feats) if live else None)
            inss[-1].priors = []                                            # the host packs none: the device writes them
        r.inp = mi.pack_inputs(inss, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP)
        with torch.cuda.stream(r.stream):
            for k, v in r.inp.items():
                r.di[k].copy_(torch.from_numpy(v))
            for k, v in r.o.items():
                v.fill_(OUT_FILL[k])
        if self.obs is not None:
            self.prior_rows()
        r.prior = not null_priors
        r.enqueue(window=W)
        r.prior = True
        dev.update(mr.AFTER_INSERT, r.d, r.o["status"], r.di["outlier_mp_id"], r.di["n_outlier"], OUTLIER_CAP)
        if self.obs is not None:
            self.obs_update(mr.AFTER_INSERT, r.o["status"])
        out = r.results()
        pri = {k: r.di[k].cpu().numpy() for k in PRIOR + ("n_prior",)}
        mst = dev.status.cpu().numpy()
        ost, pst = self.ostatus.cpu().numpy(), self.pstatus.cpu().numpy()
        for b, (it, ev) in enumerate(zip(items, evs)):
            live = ev is not None and it.window == W
            where = "insert call of window %d, step %d" % (W, self.step)
            if self.obs is not None:                                        # the prior arrays: the walk's and the model's
                got = priors_of(pri, b)
                ps, walk_pri = oa.prior_rows(it.st, [f[0] for f in inss[b].feats], sorted(it.w.mps), it.a, PRIOR_CAP)
                assert pst[b] == ps and oa.same_priors(got, walk_pri), (it.spec, where, pst[b], ps)
                if live and not it.st.err:
                    assert oa.same_priors(got, wants[b]), (it.spec, where)
                    it.seen["priors"] += bool(got); it.seen["prior_rows"] += len(got)
                it.digest(*[pri[k][b, :len(got)] for k in PRIOR], pri["n_prior"][b])
                inss[b].priors = [] if null_priors else got
            if it.st.err and live:                                          # a stale item: the chain of this history ends here
                assert ost[b] == it.st.err and oa.same(self.obs.get(b), it.st.arrays(it.a)) is None
                it.gen = iter(())
                continue
            w_after, rw = check_item(r, self.host, out, b, it.w, inss[b], window=W)
            before = it.st.arrays(it.a)
            st = mr.update(chain, it.a, mr.AFTER_INSERT, tables_of(out, b), rw["status"], outlier_ids=inss[b].outlier_ids, caps=self.arch_caps)
            assert mst[b] == st, (it.spec, where, st)
            if self.obs is not None:
                so = oa.update(it.st, oa.AFTER_INSERT, tables_full(out, b), rw["status"], st, it.a)
                assert ost[b] == so, (it.spec, where, ost[b], so)
            if not live or ev.kind == "refused":
                assert rw["status"] == mi.INVALID and st == mr.SKIPPED and (self.obs is None or so == (it.st.err or oa.SKIPPED))
            elif ev.kind == "capacity":                                     # the back end took the key-frame, the map archive could not: the store is stale
                assert rw["status"] == mi.OK and st == mr.CAPACITY
                if self.obs is not None:
                    got = self.obs.get(b)
                    assert so == oa.INVALID and got["error"] == oa.INVALID and oa.same(dict(got, error=0), before) is None
                    it.seen["stale"] += 1
                it.gen = iter(())
                continue
            else:
                rm = it.m.insert_keyframe(ev.ins)
                assert rw["status"] == rm["status"] == mi.OK and st == mr.UPDATED
                it.w = w_after
                if self.obs is not None and so == oa.CAPACITY:
                    it.capacity_at = ("insert", ev.ins.kf_id)
                    assert oa.same(dict(self.obs.get(b), error=0), before) is None      # every byte kept
                    continue
                assert self.obs is None or so == oa.UPDATED or null_priors, (it.spec, where, so)
            if it.spec and it.m.all_kfs and not it.st.err:
                self.check_state(it, b, out, where)
        self.host = {k: out[k] for k in self.host}
        return wants

    def optimise_call(self, evs):
        r, dev, chain, items, B = self.r, self.dev, self.pkg.chain, self.items, self.B
        p = lambda t: t.data_ptr()
        oo = self.oo
        opts = [next(it.gen, None) if (ev is not None and ev.kind != "capacity") else None for it, ev in zip(items, evs)]
        assert all(o is None or o.kind == "optimize" for o in opts)
        r.h.optimize_batch(*[p(r.d[k]) for k in TABLE_ARGS], B, T.K, *[p(oo[k]) for k in OPT_OUT])
        dev.update(mr.AFTER_OPTIMIZE, r.d, oo["status"], report=oo["mp_report"])
        if self.obs is not None:
            self.obs_update(mr.AFTER_OPTIMIZE, oo["status"], oo["obs_report"])
        after = self.read_tables()
        rep = {k: v.cpu().numpy() for k, v in oo.items()}
        mst, ost = dev.status.cpu().numpy(), self.ostatus.cpu().numpy()
        flats = {}
        for b, (it, ev) in enumerate(zip(items, opts)):
            where = "optimise of step %d" % self.step
            if ev is None:
                if not it.spec:
                    assert rep["status"][b] == br.EMPTY and mst[b] == mr.SKIPPED and (self.obs is None or ost[b] == oa.SKIPPED)
                elif it.st.err:
                    assert ost[b] == it.st.err
                continue
            t_in = tables_of(self.host, b)
            flat = flats[b] = r.h.debug_flat(b)

            def poses(b=b):
                return {int(k): after["kf_pose"][b, i] for i, k in enumerate(after["kf_id"][b, :int(after["n_kf"][b])])}

            def points(b=b, t_in=t_in, flat=flat):
                x = r.h.debug_solved(b)[1]
                return {int(t_in["mp_id"][row]): x[j] for j, row in enumerate(flat["pt_src"])}

            rm = it.m.optimize(ev.flags, poses, points)
            rw = br.walk(it.w, lambda *a, b=b: r.h.debug_solved(b))
            assert rep["status"][b] == rw["status"] == rm["status"], (it.spec, where)
            n_obs = len(t_in["obs_mp"])
            if rm["status"] == br.DONE:
                assert np.array_equal(rep["obs_report"][b, :n_obs], rm["obs_report"]), (it.spec, where)
            st = mr.update(chain, it.a, mr.AFTER_OPTIMIZE, tables_of(after, b), rw["status"], mp_report=rep["mp_report"][b], caps=self.arch_caps,
                           left_pos=rw["left_pos"])
            assert mst[b] == st == (mr.UPDATED if rm["status"] == br.DONE else mr.SKIPPED), (it.spec, where)
            if self.obs is not None:
                before = it.st.arrays(it.a)
                so = oa.update(it.st, oa.AFTER_OPTIMIZE, tables_full(after, b), rw["status"], st, it.a, obs_report=rep["obs_report"][b])
                assert ost[b] == so, (it.spec, where, ost[b], so)
                if so == oa.CAPACITY:
                    it.capacity_at = ("optimize", max(it.m.all_kfs))
                    assert oa.same(dict(self.obs.get(b), error=0), before) is None
                    it.gen = iter(())
                    continue
            self.check_state(it, b, after, where)
        self.host = after
        return flats

    def run(self, stop=lambda chain: False):
        while True:
            evs = self.next_events()
            if all(ev is None for ev in evs):
                break
            for W in self.windows:
                self.insert_call(W, evs)
            if all(ev is None or ev.kind == "capacity" for ev in evs) or stop(self):
                break
            self.optimise_call(evs)
            self.step += 1
            if stop(self):
                break
        return self.items


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. histories with the device's own priors

@pytest.mark.parametrize("n", range(len(H.BATCHES)))
def test_six_histories_with_the_device_s_own_priors(api, pkg, oracle, n):
    specs = H.BATCHES[n]
    caps = H.caps_for(pkg, oracle, specs)
    items = Chain(api, pkg, list(specs), caps).run()
    seen = {k: sum(it.seen[k] for it in items) for k in items[0].seen}
    print("batch %d:" % n, seen, [it.st.seen for it in items])
    for it in items:
        assert len(it.m.all_kfs) == it.spec[2] and it.capacity_at is None
    assert seen["stale"] == sum("capacity" in s[4] for s in specs) == 1
    assert seen["priors"] >= 10 and sum(it.st.seen["returned"] for it in items) >= 35 and sum(it.st.seen["left_optimize"] for it in items) >= 30


def test_items_do_not_depend_on_slot_or_neighbours(api, pkg, oracle):
    two = [H.BATCHES[0][1], H.BATCHES[0][3]]                                # a window of 3 with a correction, a window of 2 with an EMPTY optimise
    caps = tuple(v + 4 for v in H.caps_for(pkg, oracle, two))
    first = Chain(api, pkg, [two[0], two[1], None], caps).run()
    second = Chain(api, pkg, [None, two[1], two[0]], caps).run()
    assert first[0].sha.hexdigest() == second[2].sha.hexdigest() and first[1].sha.hexdigest() == second[1].sha.hexdigest()
    assert first[0].sha.hexdigest() != first[1].sha.hexdigest()
    for it in (first[2], second[0]):
        assert not it.st.t_id and not it.st.seg and it.st.used == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. reclaim

@pytest.mark.parametrize("seed, cap", [(116, 47), (149, 54), (201, 67)])
def test_reclaim_at_the_history_s_own_maximum_of_live_rows(api, pkg, oracle, seed, cap):
    """row_cap = the most live rows the history ever holds (tests/test_obs_archive_ref.py holds the walk to these numbers and to the 136, 173 and 132 rows
    a pool that only appends would have used): the run must finish, with a reclaim"""
    spec = next(s for s in T.HISTORIES if s[0] == seed)
    caps = tuple(v + 2 for v in T.caps_of(pkg, oracle, spec))
    ch = Chain(api, pkg, [spec, None], caps, row_cap=cap)
    it, other = ch.run()
    got = ch.obs.get(0)
    assert it.capacity_at is None and len(it.m.all_kfs) == spec[2] and it.st.seen["most_live"] == cap
    assert got["n_reclaims"] == it.st.n_reclaim >= 1 and got["rows_in_use"] <= cap
    print(seed, "reclaims", got["n_reclaims"], "rows in use", got["rows_in_use"], "of", cap)
    # one row less: the walk names the event, the device answers MYSLAM_ERR_CAPACITY there, keeps every byte and stays in error
    ch = Chain(api, pkg, [spec, None], caps, row_cap=cap - 1)
    it, other = ch.run(stop=lambda c: c.items[0].capacity_at is not None)
    assert it.capacity_at is not None and it.st.err == oa.CAPACITY
    before = ch.obs.get(0)
    assert before["error"] == oa.CAPACITY
    ch.prior_rows()
    ch.obs_update(mr.AFTER_INSERT, ch.r.o["status"])
    ch.r.stream.synchronize()
    assert ch.pstatus.cpu().numpy().tolist() == [oa.CAPACITY, 0] and ch.r.di["n_prior"].cpu().numpy().tolist() == [0, 0]
    assert ch.ostatus.cpu().numpy()[0] == oa.CAPACITY and oa.same(ch.obs.get(0), before) is None
    assert oa.same(ch.obs.get(1), oa.Store().arrays(other.a)) is None      # the second item: untouched
    print(seed, "row_cap", cap - 1, "capacity at", it.capacity_at)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. beyond one block pass: 300 stored points, 270 of them named at once, 300 points leaving at once, a reclaim

class MapView:
    """the map archive's ids and states of one item, read from the device: what the walk needs of it"""

    def __init__(self, got):
        self.mp_id, self.mp_state = [int(i) for i in got["mp_id"]], [int(s) for s in got["mp_state"]]


def big_case(chain):
    """-> (the back end's map, the stored segments [(id, rows)], the key-frame).  Window 2: key-frame 10 at x = -5 holds map points 1000..1299 alone (1 or 2
    ACTIVE rows each), key-frame 20 at x = 0 sees 16 exact points 2000..2015; the new key-frame 30 at x = 1 makes key-frame 10, the farthest, leave and
    with it all 300 points, alive.  Map points 100..399 are stored with 1 to 3 rows of key-frames 1..3; 280 features name 270 of them, ten twice."""
    rng = np.random.default_rng(0x0B5A)
    m = br.Map()
    poses = {10: mi.shifted(-5.0), 20: mi.shifted(0.0)}
    for k, p in poses.items():
        m.kfs[k] = p
    tag = [0]

    def obs_at(kf, pose, pw):
        uv, _ = wm.project(chain, T.K, pose, pw)
        tag[0] += 1
        return br.Obs(kf, np.float32(uv[0]), np.float32(uv[1]), False, tag[0])

    for j in range(300):
        mp = br.MapPoint(1000 + j, (rng.uniform(-8, -2), rng.uniform(-1, 1), rng.uniform(8, 20)))
        for _ in range(1 + j % 2):
            o = obs_at(10, poses[10], mp.pos); mp.obs.append(o); mp.active_obs.append(o)
        m.mps[mp.id] = mp
    for j in range(16):
        mp = br.MapPoint(2000 + j, (rng.uniform(-2, 3), rng.uniform(-1, 1), rng.uniform(8, 20)))
        o = obs_at(20, poses[20], mp.pos); mp.obs.append(o); mp.active_obs.append(o)
        m.mps[mp.id] = mp
    stored, pos = [], {}
    for j in range(300):
        pos[100 + j] = (rng.uniform(-2, 4), rng.uniform(-1, 1), rng.uniform(8, 20))
        rows = []
        for n in range(1 + j % 3):
            tag[0] += 1
            rows.append((1 + n, np.float32(rng.uniform(10, 1200)), np.float32(rng.uniform(10, 370)), tag[0], br.OUTLIER if (j + n) % 7 == 0 else 0))
        stored.append((100 + j, rows))
    new_pose = mi.shifted(1.0)
    named = [100 + j for j in range(300) if j % 10 != 3]                    # 270 of the 300, ten of them twice
    feats = []
    for mid in named + named[5:105:10]:
        uv, _ = wm.project(chain, T.K, new_pose, pos[mid])
        tag[0] += 1
        feats.append((mid, tuple(pos[mid]), (np.float32(uv[0]), np.float32(uv[1])), tag[0], False))
    feats = [feats[i] for i in rng.permutation(len(feats))]
    assert len(named) == 270 and len(feats) == 280
    return m, stored, pos, mi.Insert(30, new_pose, feats)


def test_beyond_one_block_pass(api, pkg):
    import torch
    chain = pkg.chain
    m, stored, pos, ins = big_case(chain)
    feat_cap, prior_cap, row_cap = 320, 640, 700
    be_caps = (4, 640, 2048)
    # the map archive: every key-frame and point the item ever saw, by its own walk; the stored points were active under key-frames 1..3
    a = mr.Archive()
    w0 = br.Map()
    for k in (1, 2, 3):
        w0.kfs[k] = mi.shifted(-9.0 + k)
    for mid, rows in stored:
        mp = br.MapPoint(mid, pos[mid])
        mp.obs = [br.Obs(r[0], r[1], r[2], bool(r[4]), r[3]) for r in rows]; mp.active_obs = list(mp.obs)
        w0.mps[mid] = mp
    arch_caps = (8, 8, 700)
    assert mr.update(chain, a, mr.AFTER_INSERT, br.pack(w0), 0, caps=arch_caps) == mr.UPDATED
    assert mr.update(chain, a, mr.AFTER_INSERT, br.pack(m), 0, caps=arch_caps) == mr.UPDATED
    rows_of = lambda mp: [(o.kf, o.u, o.v, o.tag, br.OUTLIER if o.outlier else 0) for o in mp.obs]
    st = oa.Store.loaded(row_cap, stored, sorted(m.mps), [rows_of(m.mps[i]) for i in sorted(m.mps)])
    ins.priors = []
    r = Run(api, [m], [ins], 2, 0.2, caps=(be_caps, feat_cap, prior_cap, 4))
    dev = Dev(api, 1, arch_caps, be_caps, r.stream)
    arr = a.arrays()
    arr["mp_win_mask"][:len(stored)] = 0                                    # the stored points' bits are of the three key-frames' window: none of it is left
    dev.h.load(0, *[arr[k] for k in H.LOAD])
    obs = api.ObsArchive(dev.h, 1, be_caps[2], row_cap, stream=r.stream.cuda_stream)
    obs.load(0, *st.load_args(a))
    assert oa.same(obs.get(0), st.arrays(a)) is None
    full = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
    oo = dict(obs_report=full((1, be_caps[2]), torch.uint8), mp_report=full((1, be_caps[1]), torch.uint8), new_outlier=full((1, be_caps[1]), torch.int32),
              n_new=full((1,), torch.int32), obs_chi2=full((1, be_caps[2]), torch.float64), rounds=full((1,), torch.int32), n_out=full((1,), torch.int32),
              status=full((1,), torch.int32))
    ostatus, pstatus = full((1,), torch.int32, STATUS_FILL), full((1,), torch.int32, STATUS_FILL)
    r.stream.wait_stream(torch.cuda.current_stream())
    p = lambda t: t.data_ptr()
    d, di = r.d, r.di
    obs.prior_rows_batch(p(di["feat_mp_id"]), p(di["n_feat"]), feat_cap, p(d["mp_id"]), p(d["n_mp"]), be_caps[1], 1, *[p(di[k]) for k in PRIOR], p(di["n_prior"]),
                         prior_cap, p(pstatus))
    r.enqueue()
    dev.update(mr.AFTER_INSERT, d, r.o["status"], di["outlier_mp_id"], di["n_outlier"], 4)
    obs.update_batch(mr.AFTER_INSERT, *[p(d[k]) for k in TABLE_ARGS], *be_caps, p(r.o["status"]), p(dev.status), None, 1, p(ostatus))
    out = r.results()
    pri = {k: di[k].cpu().numpy() for k in PRIOR + ("n_prior",)}
    got_pri = priors_of(pri, 0)
    ps, walk_pri = oa.prior_rows(st, [f[0] for f in ins.feats], sorted(m.mps), a, prior_cap)
    assert pstatus.cpu().numpy()[0] == ps == oa.OK and oa.same_priors(got_pri, walk_pri) and len({q[0] for q in got_pri}) == 270 and len(got_pri) > 256
    ins.priors = got_pri
    w_after, rw = check_item(r, r.host, out, 0, m, ins)
    assert rw["status"] == mi.OK and rw["removed_kf_id"] == 10 and len(w_after.mps) == 286
    assert dev.status.cpu().numpy()[0] == mr.UPDATED
    view = MapView(dev.h.get(0))
    so = oa.update(st, oa.AFTER_INSERT, tables_full(out, 0), rw["status"], mr.UPDATED, view)
    got = obs.get(0)
    assert ostatus.cpu().numpy()[0] == so == oa.UPDATED and oa.same(got, st.arrays(view)) is None, oa.same(got, st.arrays(view))
    assert got["n_reclaims"] == 1 and len(got["seg_mp_id"]) == 330 and st.seen["left_insert"] == 300 and st.seen["returned"] == 270
    # the optimise and its update: 286 points in the table, more than one pass of the workgroup
    r.h.optimize_batch(*[p(d[k]) for k in TABLE_ARGS], 1, T.K, *[p(oo[k]) for k in OPT_OUT])
    dev.update(mr.AFTER_OPTIMIZE, d, oo["status"], report=oo["mp_report"])
    obs.update_batch(mr.AFTER_OPTIMIZE, *[p(d[k]) for k in TABLE_ARGS], *be_caps, p(oo["status"]), p(dev.status), p(oo["obs_report"]), 1, p(ostatus))
    r.stream.synchronize()
    after = {k: v.cpu().numpy() for k, v in d.items()}
    rep = {k: v.cpu().numpy() for k, v in oo.items()}
    assert rep["status"][0] == br.DONE and dev.status.cpu().numpy()[0] == mr.UPDATED
    view = MapView(dev.h.get(0))
    so = oa.update(st, oa.AFTER_OPTIMIZE, tables_full(after, 0), 0, mr.UPDATED, view, obs_report=rep["obs_report"][0])
    got = obs.get(0)
    assert ostatus.cpu().numpy()[0] == so == oa.UPDATED and oa.same(got, st.arrays(view)) is None, oa.same(got, st.arrays(view))
    print("after the optimise: table points", len(got["table_mp_id"]), "stored", len(got["seg_mp_id"]), "culled rows", int((rep["obs_report"][0] == 1).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. edges

def test_call_level_errors(api):
    import torch
    m = api.MapArchive(2, 8, 8, 64, 16)
    with pytest.raises(api.MyslamError) as e:
        api.ObsArchive(m, 3, 64, 32)                                        # more items than the map holds
    assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.MyslamError):
        api.ObsArchive(m, 2, 0, 32)
    h = api.ObsArchive(m, 2, 64, 32)
    assert h.launches_per_update() == 1
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    q, qs = x.data_ptr(), status.data_ptr()
    tables = [q] * 13
    good_u = [api.MAP_AFTER_OPTIMIZE] + tables + [4, 16, 64, q, q, q, 2, qs]
    good_p = [q, q, 8, q, q, 16, 2, q, q, q, q, q, q, 8, qs]

    def code(fn, args):
        with pytest.raises(api.MyslamError) as e:
            fn(*args)
        return e.value.code

    def with_(args, i, v):
        return args[:i] + [v] + args[i + 1:]

    for i in (1, 3, 4, 7, 8, 9, 10, 11, 12, 13, 17, 18, 19, 21):        # every required pointer; the report after an optimise
        assert code(h.update_batch, with_(good_u, i, None)) == api.ERR_INVALID, i
    assert code(h.update_batch, with_(good_u, 0, 2)) == api.ERR_INVALID                 # an unknown mode
    assert code(h.update_batch, with_(good_u, 15, 17)) == api.ERR_INVALID               # not the map's backend_mp_cap
    assert code(h.update_batch, with_(good_u, 16, 65)) == api.ERR_INVALID               # not the handle's be_obs_cap
    assert code(h.update_batch, with_(good_u, 20, 3)) == api.ERR_CAPACITY               # a batch beyond the handle's
    for i in (0, 1, 3, 4, 7, 8, 9, 10, 11, 12, 14):
        assert code(h.prior_rows_batch, with_(good_p, i, None)) == api.ERR_INVALID, i
    assert code(h.prior_rows_batch, with_(good_p, 5, 15)) == api.ERR_INVALID
    assert code(h.prior_rows_batch, with_(good_p, 6, 3)) == api.ERR_CAPACITY
    h.update_batch(*with_(with_(good_u, 0, api.MAP_AFTER_INSERT), 19, None))             # no report after an insert; x is all zeros: statuses 0, nk = 0
    h.update_batch(*with_(good_u, 20, 0))                                                 # an empty batch
    torch.cuda.synchronize()
    assert status.cpu().tolist()[:2] == [api.ERR_INVALID] * 2                            # an empty key-frame table after a call that answered 0: stale
    # load: what the header lists
    one = lambda: ([5], [1], [7], [(1.0, 2.0)], [9], [0])
    assert code(h.load, [0] + list(one())) == api.ERR_INVALID                            # an id the map does not hold
    assert code(h.load, [2] + list(one())) == api.ERR_INVALID                            # an item beyond the handle's
    g = h.get(0)
    assert g["error"] == api.ERR_INVALID and len(g["seg_mp_id"]) == 0                    # the update above found an empty key-frame table: stale
    m.load(0, [1], [mi.IDENT], [], [], np.zeros((0, 7)), [5, 6], np.zeros((2, 3)), [0, 0], [0, 2])
    h.load(0, *one())
    g = h.get(0)
    assert g["error"] == 0 and g["seg_mp_id"].tolist() == [5] and g["row_kf_id"].tolist() == [7] and g["rows_in_use"] == 1
    assert code(h.load, [0, [6], [1], [7], [(1.0, 2.0)], [9], [0]]) == api.ERR_INVALID   # an erased point
    assert code(h.load, [0, [5], [1], [7], [(1.0, 2.0)], [9], [1]]) == api.ERR_INVALID   # ACTIVE is never stored
    assert code(h.load, [0, [5], [2], [7], [(1.0, 2.0)], [9], [0]]) == api.ERR_INVALID   # counts that do not sum to the rows
    assert code(h.load, [0, [5], [33], [7] * 33, [(1.0, 2.0)] * 33, [9] * 33, [0] * 33]) == api.ERR_CAPACITY
    assert oa.same(h.get(0), g) is None                                                 # a refused load keeps every byte


def seed_116(api, pkg, oracle, row_cap=ROW_CAP, with_obs=True):
    spec = next(s for s in T.HISTORIES if s[0] == 116)
    return Chain(api, pkg, [spec, None, None], tuple(v + 2 for v in T.caps_of(pkg, oracle, spec)), row_cap=row_cap, with_obs=with_obs)


def run_to_first_return(ch):
    """-> (events, the model's priors) of the first key-frame that brings a stored point back; everything before it has run"""
    while True:
        evs = ch.next_events()
        want = ch.items[0].m.priors_for(evs[0].ins.feats)
        if want:
            return evs, want
        ch.insert_call(ch.windows[0], evs, null_priors=ch.obs is None)
        ch.optimise_call(evs)
        ch.step += 1


def test_null_priors_for_a_stored_point_make_the_item_stale_until_a_load(api, pkg, oracle):
    ch = seed_116(api, pkg, oracle)
    it = ch.items[0]
    evs, want = run_to_first_return(ch)
    assert len(it.m.all_kfs) == 3                                           # its 4th key-frame
    before = ch.obs.get(0)
    ch.insert_call(ch.windows[0], evs, null_priors=True)                    # the walk answers INVALID and so must the device (checked in the call)
    assert it.st.err == oa.INVALID and ch.ostatus.cpu().numpy().tolist() == [oa.INVALID, oa.SKIPPED, oa.SKIPPED]
    assert oa.same(dict(ch.obs.get(0), error=0), before) is None            # every byte kept
    for _ in range(2):                                                      # and it stays so
        ch.prior_rows()
        ch.obs_update(mr.AFTER_INSERT, ch.r.o["status"])
        ch.r.stream.synchronize()
        assert ch.pstatus.cpu().numpy()[0] == oa.INVALID and ch.r.di["n_prior"].cpu().numpy()[0] == 0 and ch.ostatus.cpu().numpy()[0] == oa.INVALID
    # load: the segments the model holds now and the mirror of the table as it stands (a row's observer by its tag, which the model knows)
    out = ch.read_tables()
    t = tables_full(out, 0)
    kf_of = {o.tag: int(o.kf) for mp in it.m.all_mps.values() for o in mp.obs}
    segs = _segments_of(t, kf_of)
    view = MapView(ch.dev.h.get(0))
    stored = [(mid, [(int(o.kf), o.u, o.v, o.tag, br.OUTLIER if o.outlier else 0) for o in mp.obs]) for mid, mp in sorted(it.m.all_mps.items())
              if mid not in [int(i) for i in t["mp_id"]]]
    st = oa.Store.loaded(ROW_CAP, stored, t["mp_id"], segs)
    ch.obs.load(0, *st.load_args(view))
    got = ch.obs.get(0)
    assert got["error"] == 0 and got["n_reclaims"] == 0 and oa.same(got, st.arrays(view)) is None
    ch.prior_rows()
    ch.r.stream.synchronize()
    assert ch.pstatus.cpu().numpy()[0] == oa.OK


def _segments_of(t, kf_of):
    out = [[] for _ in t["mp_id"]]
    for r, m in enumerate(t["obs_mp"]):
        out[int(m)].append((kf_of[int(t["obs_tag"][r])], t["obs_uv"][r][0], t["obs_uv"][r][1], int(t["obs_tag"][r]), int(t["obs_flags"][r]) & br.OUTLIER))
    return out


def test_prior_cap_one_short_for_one_item_of_three(api, pkg, oracle):
    """three items hold the same stored point of 2 rows and are asked for it; prior_cap 2 holds it, and the item that is asked for a second point of
    1 row is one short: MYSLAM_ERR_CAPACITY, a count of 0, nothing written, not sticky"""
    import torch
    m = api.MapArchive(3, 8, 8, 16, 8)
    h = api.ObsArchive(m, 3, 32, 16)
    for b in range(3):
        m.load(b, [1], [mi.IDENT], [], [], np.zeros((0, 7)), [5, 6, 9], np.zeros((3, 3)), [0, 0, 0], [0, 1, 0])
        h.load(b, [5, 6], [2, 1], [1, 2, 3], [(1.0, 2.0), (3.0, 4.0), (5.0, 6.0)], [11, 12, 13], [0, 2, 0])
    feat = torch.tensor([[5, -1, 5, 77], [6, 5, 5, 9], [5, 4, -1, -1]], dtype=torch.int64, device="cuda")
    nf = torch.tensor([4, 4, 2], dtype=torch.int32, device="cuda")
    be_id = torch.full((3, 8), 9, dtype=torch.int64, device="cuda"); be_n = torch.tensor([1, 1, 0], dtype=torch.int32, device="cuda")
    o = dict(mp=torch.full((3, 2), -64, dtype=torch.int64, device="cuda"), kf=torch.full((3, 2), -63, dtype=torch.int64, device="cuda"),
             uv=torch.full((3, 2, 2), -4.5, dtype=torch.float32, device="cuda"), tag=torch.full((3, 2), -62, dtype=torch.int32, device="cuda"),
             fl=torch.full((3, 2), 0xAB, dtype=torch.uint8, device="cuda"), n=torch.full((3,), -5, dtype=torch.int32, device="cuda"),
             st=torch.full((3,), STATUS_FILL, dtype=torch.int32, device="cuda"))
    p = lambda t: t.data_ptr()
    torch.cuda.synchronize()
    for _ in range(2):
        h.prior_rows_batch(p(feat), p(nf), 4, p(be_id), p(be_n), 8, 3, p(o["mp"]), p(o["kf"]), p(o["uv"]), p(o["tag"]), p(o["fl"]), p(o["n"]), 2, p(o["st"]))
        torch.cuda.synchronize()
        assert o["st"].cpu().tolist() == [0, api.ERR_CAPACITY, 0] and o["n"].cpu().tolist() == [2, 0, 2]
        assert o["mp"].cpu().tolist() == [[5, 5], [-64, -64], [5, 5]] and o["kf"].cpu().tolist() == [[1, 2], [-63, -63], [1, 2]]
        assert o["tag"].cpu().tolist() == [[11, 12], [-62, -62], [11, 12]] and o["fl"].cpu().tolist() == [[0, 2], [0xAB, 0xAB], [0, 2]]
        assert o["uv"].cpu().tolist() == [[[1.0, 2.0], [3.0, 4.0]], [[-4.5, -4.5]] * 2, [[1.0, 2.0], [3.0, 4.0]]]
    assert all(h.get(b)["error"] == 0 for b in range(3))


def test_a_skipped_item_keeps_every_byte(api, pkg, oracle):
    ch = seed_116(api, pkg, oracle)
    for _ in range(3):
        evs = ch.next_events()
        ch.insert_call(ch.windows[0], evs)
        ch.optimise_call(evs)
        ch.step += 1
    before = ch.obs.get(0)
    assert len(before["seg_mp_id"]) > 0
    ch.insert_call(ch.windows[0], [None, None, None])                       # parked: the back end refuses, the map skips, and so does the store
    assert ch.ostatus.cpu().numpy().tolist() == [oa.SKIPPED] * 3 and oa.same(ch.obs.get(0), before) is None


def test_three_recorded_key_frames_replayed_equal_the_eager_run(api, pkg, oracle):
    """three key-frames of seed 116 that bring points back (its 6th to 8th: no correction lies between them), each as prior_rows -> insert -> map update
    -> obs update -> optimise -> map update -> obs update, recorded as ONE graph on inputs that lie on the device, and replayed once: the prior arrays
    of each key-frame, every table and the store must be what the eager run left"""
    import torch
    eager, rec = seed_116(api, pkg, oracle), seed_116(api, pkg, oracle)
    for c in (eager, rec):
        for _ in range(5):
            evs = c.next_events()
            c.insert_call(c.windows[0], evs)
            c.optimise_call(evs)
            c.step += 1
    p = lambda t: t.data_ptr()

    def step(c):
        c.prior_rows()
        c.r.enqueue(window=c.windows[0])
        c.dev.update(mr.AFTER_INSERT, c.r.d, c.r.o["status"], c.r.di["outlier_mp_id"], c.r.di["n_outlier"], OUTLIER_CAP)
        c.obs_update(mr.AFTER_INSERT, c.r.o["status"])
        c.r.h.optimize_batch(*[p(c.r.d[k]) for k in TABLE_ARGS], c.B, T.K, *[p(c.oo[k]) for k in OPT_OUT])
        c.dev.update(mr.AFTER_OPTIMIZE, c.r.d, c.oo["status"], report=c.oo["mp_report"])
        c.obs_update(mr.AFTER_OPTIMIZE, c.oo["status"], c.oo["obs_report"])

    inputs, pri_e, returned = [], [], 0
    for n in range(3):
        evs = eager.next_events()
        assert evs[0].kind == "insert" and not eager.corrected
        wants = eager.insert_call(eager.windows[0], evs)
        inputs.append({k: torch.from_numpy(v.copy()).cuda() for k, v in eager.r.inp.items()})
        pri_e.append({k: eager.r.di[k].cpu().numpy() for k in PRIOR + ("n_prior",)})
        eager.optimise_call(evs)
        eager.step += 1
        returned += len(wants[0])
    assert returned > 0 and all(q["n_prior"][0] > 0 for q in pri_e)
    torch.cuda.synchronize()
    own = rec.r.di

    def body():
        for di in inputs:
            rec.r.di = di
            step(rec)

    with torch.cuda.stream(rec.r.stream):
        g = api.StepGraph.record(rec.r.stream.cuda_stream, [], body)
    rec.r.di = own
    assert g.node_count() >= 3 * (rec.obs.launches_per_update() * 2 + 1 + 1 + 2 + 3)
    g.launch(rec.r.stream.cuda_stream)
    rec.r.stream.synchronize()
    for n in range(3):
        for k in PRIOR + ("n_prior",):
            assert inputs[n][k].cpu().numpy().tobytes() == pri_e[n][k].tobytes(), (n, k)
    for k in rec.r.d:
        assert rec.r.d[k].cpu().numpy().tobytes() == eager.r.d[k].cpu().numpy().tobytes(), k
    assert rec.ostatus.cpu().numpy().tolist() == eager.ostatus.cpu().numpy().tolist() == [oa.UPDATED, oa.SKIPPED, oa.SKIPPED]
    assert oa.same(rec.obs.get(0), eager.obs.get(0)) is None and mr.same(rec.dev.h.get(0), eager.dev.h.get(0)) is None


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. the gap itself: without prior rows a returning point is a FREE landmark on the device and a FIXED one in the reference

def test_the_gap_a_returning_point_without_prior_rows_is_a_free_landmark(api, pkg, oracle):
    """seed 116 on the back end and the map archive alone, NULL priors on every insert, as a device-only stream ran before the observation archive
    existed.  At its first return, its 4th key-frame, the model's front observation of the point lies outside the window: src/backend.cpp:175-177 fixes
    it.  The device opened a fresh segment whose first row is the new key-frame's, and its flatten leaves the landmark free."""
    ch = seed_116(api, pkg, oracle, with_obs=False)
    it = ch.items[0]
    evs, want = run_to_first_return(ch)
    assert len(it.m.all_kfs) == 3
    back = sorted({q[0] for q in want})
    r = ch.r
    inss = [evs[0].ins, PARKED, PARKED]
    for i in inss:
        i.priors = []
    r.inp = mi.pack_inputs(inss, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP)
    with ch.torch.cuda.stream(r.stream):
        for k, v in r.inp.items():
            r.di[k].copy_(ch.torch.from_numpy(v))
    r.prior = False
    r.enqueue(window=ch.windows[0])
    out = r.results()                                                       # the table as the optimise will find it: pt_src names its rows
    p = lambda t: t.data_ptr()
    r.h.optimize_batch(*[p(r.d[k]) for k in TABLE_ARGS], ch.B, T.K, *[p(ch.oo[k]) for k in OPT_OUT])
    r.stream.synchronize()
    assert out["status"][0] == mi.OK and ch.oo["status"].cpu().numpy()[0] == br.DONE
    flat = r.h.debug_flat(0)
    ids = [int(out["mp_id"][0, row]) for row in flat["pt_src"]]
    it.m.insert_keyframe(evs[0].ins)
    mflat, _, slot_mps = br.flatten(it.m.active_map())
    fixed_model = {mp.id: int(f) for mp, f in zip(slot_mps, mflat["fixed"])}
    gap = [mid for mid in back if mid in ids and fixed_model.get(mid) == 1 and flat["fixed"][ids.index(mid)] == 0]
    print("returning points", back, "fixed in the model, free on the device:", gap)
    assert gap and gap == [mid for mid in back if mid in ids]
