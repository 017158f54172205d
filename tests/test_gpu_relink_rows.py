"""The rows of the re-link on the device (include/myslam_hip.h, RE-LINK): myslam_relink_stage_batch, myslam_relink_backend_batch, myslam_map_relink_batch,
myslam_map_update_batch(MYSLAM_MAP_AFTER_RELINK), myslam_relink_obs_update_batch and myslam_relink_first_kf_batch against the walks of
tests/relink_ref.py, which tests/test_relink_ref.py holds against the object model over whole histories.  Every re-link of the twelve histories that a
key-frame follows is one item: the state the walks had before it is loaded (the back end's tables, the map archive, the observation archive), the calls
run in batches of up to six items of one window, and after them every byte below the counts of the thirteen tables, MapArchive.get, ObsArchive.get, the
link list of the moved rows and first_kf equal the walks.  Then the device goes on by itself: prior_rows, the next key-frame's insert and the two
updates, compared again, so a merged target that returns is the fixed landmark of the next window.  Needs an MI355X."""
import copy

import numpy as np
import pytest

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
import obs_archive_ref as oa
import relink_ref as rr
import whole_map_model as wm
from test_gpu_map_archive import Dev
from test_gpu_map_histories import BE_CAPS, FEAT_CAP, LOAD, OUTLIER_CAP, PRIOR_CAP
from test_gpu_map_insert import OUT_FILL, TABLE_ARGS, Run
from test_whole_map_model import HISTORIES, K

pytestmark = pytest.mark.gpu

O, F = rr.OUT_CAP, rr.FEAT_CAP
ARCH_CAPS = (24, 24, 640)
ROW_CAP = 400
SENT = -4242
PRIOR = ("prior_mp_id", "prior_kf_id", "prior_uv", "prior_tag", "prior_flags")
READ_ARGS = ("kf_id", "n_kf", "mp_id", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")


class DevArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


@pytest.fixture(scope="module")
def cases(pkg):
    out = []
    for spec in HISTORIES:
        out += [c for c in rr.replay_rows(pkg.chain, spec, K, record=True)["cases"] if c["next_insert"] is not None]
    return out


def loaded_store(c, row_cap):
    return oa.Store.loaded(row_cap, c["st_before"].live(c["a_before"]), c["st_before"].t_id, c["st_before"].t_rows)


def walk_relink(chain, c, row_cap=ROW_CAP, obs_cap=BE_CAPS[2], stage_cap=1 << 30):
    """the walks of one item from its recorded state -> everything the device must leave"""
    w, a, st = c["w_before"].clone(), copy.deepcopy(c["a_before"]), loaded_store(c, row_cap)
    p = c["plan"]
    stg = rr.stage(st, a, p["merge"], p["target"], p["status"], be_obs_cap=obs_cap, stage_cap=stage_cap)
    be = rr.backend_relink(w, stg, obs_cap)
    mst, state2 = rr.map_relink(np.array(a.mp_state, np.uint8), p["merge"], len(p["merge"]), O, be["status"])
    a.mp_state = [int(v) for v in state2]
    ms = mr.update(chain, a, mr.AFTER_INSERT, br.pack(w), be["status"], caps=ARCH_CAPS)
    so = rr.obs_update_relink(st, br.pack(w), be["status"], ms, a, stg)
    return dict(w=w, a=a, st=st, stage=stg, be=be, map_status=mst, update_status=ms, obs_status=so, first_kf=rr.first_kf(st, a))


class Rows:
    """a batch of recorded items on the device"""

    def __init__(self, api, pkg, items, row_cap=ROW_CAP, be_caps=BE_CAPS, stage_cap=None):
        import torch
        self.torch, self.api, self.chain, self.B, self.row_cap, self.be_caps = torch, api, pkg.chain, len(items), row_cap, be_caps
        self.window = items[0]["window"]
        self.r = r = Run(api, [c["w_before"] for c in items], self._inserts(items), self.window, 0.2, caps=(be_caps, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP))
        sp = r.stream.cuda_stream
        B = self.B
        self.dev = Dev(api, B, ARCH_CAPS, be_caps, r.stream)
        self.obs = api.ObsArchive(self.dev.h, B, be_caps[2], row_cap, stream=sp)
        self.rl = api.Relink(self.dev.h, B, O, F, be_caps[2] + row_cap if stage_cap is None else stage_cap, stream=sp)
        self.store = api.LoopKeyFrameStore(1, 8, F, stream=sp)             # holds nothing: the lists go to the pending table of every item
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.buf = dict(pairs=z((B, O, 2), torch.int32), counts=z((B,), torch.int32), outlier=z((B, O), torch.uint8), cstat=z((B,), torch.int32),
                        cur=z((B, F), torch.int32), loop=z((B, F), torch.int32), kf=z((B,), torch.int64), pend=z((B, F), torch.int32))
        for k in ("plan", "stage", "be", "map", "obs", "prior"):
            self.buf[k + "_status"] = z((B,), torch.int32)
        self.buf.update(new_row=z((B, be_caps[1]), torch.int32), first_kf=z((B, ARCH_CAPS[2]), torch.int32), n_set_rows=z((B,), torch.int32), n_set_plan=z((B,), torch.int32))
        v = self.view = self.rl.view()
        S = v.stage_cap
        t = lambda ptr, shape, ty: torch.as_tensor(DevArray(ptr, shape, ty), device="cuda")
        self.rows = dict(kf=t(v.row_kf_id, (B, S), "<i8"), tag=t(v.row_tag, (B, S), "<i4"), slot=t(v.row_slot, (B, S), "<i4"), place=t(v.row_place, (B, S), "<i4"),
                         root=t(v.row_root_id, (B, S), "<i8"), uv=t(v.row_uv, (B, S, 2), "<f4"), flags=t(v.row_flags, (B, S), "|u1"), n=t(v.n_rows, (B,), "<i4"),
                         merge=t(v.merge, (B, O, 2), "<i4"), n_merge=t(v.n_merge, (B,), "<i4"), table_rows=t(v.table_rows, (B,), "<i4"))
        self.load(items)

    @staticmethod
    def _inserts(items):
        out = []
        for c in items:
            ins = copy.deepcopy(c["next_insert"]); ins.priors = []
            out.append(ins)
        return out

    def load(self, items):
        """the recorded state of `items` into the handles and buffers this object holds (nothing is created: a recording stays valid)"""
        torch, r = self.torch, self.r
        assert len(items) == self.B and all(c["window"] == self.window for c in items)
        self.items = items
        r.host = br.pack_batch([c["w_before"] for c in items], *r.caps)
        r.inp = mi.pack_inputs(self._inserts(items), r.feat_cap, r.prior_cap, r.outlier_cap)
        for b, c in enumerate(items):
            self.dev.h.load(b, *[c["a_before"].arrays()[k] for k in LOAD])
            self.obs.load(b, *loaded_store(c, self.row_cap).load_args(c["a_before"]))
        host = dict(pairs=np.stack([c["pairs"] for c in items]), counts=np.array([c["count"] for c in items], np.int32), outlier=np.stack([c["outlier"] for c in items]),
                    cstat=np.array([c["correct_status"] for c in items], np.int32), cur=np.stack([c["cur"] for c in items]), loop=np.stack([c["loop"] for c in items]),
                    kf=np.array([c["cur_kf"] for c in items], np.int64))
        with torch.cuda.stream(r.stream):
            for k, v in r.host.items():
                r.d[k].copy_(torch.from_numpy(v))
            for k, v in r.inp.items():
                r.di[k].copy_(torch.from_numpy(v))
            for k, v in r.o.items():
                v.fill_(OUT_FILL[k])
            for k, v in host.items():
                self.buf[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
            self.buf["pend"].copy_(self.buf["cur"])
            for k, v in self.buf.items():
                if k not in host and k != "pend":
                    v.fill_(SENT)
            self.dev.status.fill_(SENT)
        torch.cuda.synchronize()

    def steps(self):
        p = lambda k: self.buf[k].data_ptr()
        d, v, B = self.r.d, self.view, self.B
        return [("plan", lambda: self.rl.plan_batch(p("pairs"), p("counts"), p("outlier"), p("cstat"), p("cur"), p("loop"), p("kf"), B, p("plan_status"))),
                ("stage", lambda: self.rl.stage_batch(self.obs, p("plan_status"), B, p("stage_status"))),
                ("backend", lambda: self.rl.backend_batch(self.r.h, *[d[k].data_ptr() for k in TABLE_ARGS], p("stage_status"), B, p("new_row"), p("be_status"))),
                ("map_relink", lambda: self.dev.h.relink_batch(v.merge, v.n_merge, O, p("be_status"), B, p("map_status"))),
                ("map_update", lambda: self.dev.update(rr.AFTER_RELINK, d, self.buf["be_status"])),
                ("obs_update", lambda: self.rl.obs_update_batch(self.obs, *[d[k].data_ptr() for k in READ_ARGS], *self.be_caps, p("be_status"),
                                                                self.dev.status.data_ptr(), B, p("obs_status"))),
                ("first_kf", lambda: self.api.Relink.first_kf_batch(self.obs, B, p("first_kf"))),
                # the current key-frame as a pending one: the moved rows' list, then the plan's
                ("links_rows", lambda: self.store.set_links_batch(v.row_kf_id, v.row_tag, v.row_slot, v.n_rows, v.stage_cap, B, p("kf"), p("pend"), p("n_set_rows"))),
                ("links_plan", lambda: self.store.set_links_batch(v.link_kf_id, v.link_tag, v.link_slot, v.n_link, F, B, p("kf"), p("pend"), p("n_set_plan")))]

    def relink(self, after=None):
        """the whole re-link; after(name) runs between the calls, on a quiet device (the per-item faults spoil a list there)"""
        for name, call in self.steps():
            call()
            if after is not None:
                self.r.stream.synchronize()
                after(name)
                self.torch.cuda.synchronize()

    def key_frame(self):
        p = lambda t: t.data_ptr()
        d, di, r = self.r.d, self.r.di, self.r
        self.obs.prior_rows_batch(p(di["feat_mp_id"]), p(di["n_feat"]), FEAT_CAP, p(d["mp_id"]), p(d["n_mp"]), self.be_caps[1], self.B, *[p(di[k]) for k in PRIOR],
                                  p(di["n_prior"]), PRIOR_CAP, p(self.buf["prior_status"]))
        r.enqueue()
        self.dev.update(mr.AFTER_INSERT, d, r.o["status"], di["outlier_mp_id"], di["n_outlier"], OUTLIER_CAP)
        self.obs.update_batch(mr.AFTER_INSERT, *[p(d[k]) for k in TABLE_ARGS], *self.be_caps, p(r.o["status"]), p(self.dev.status), None, self.B, p(self.buf["obs_status"]))

    def read(self):
        self.r.stream.synchronize()
        self.torch.cuda.synchronize()
        g = {k: v.cpu().numpy().copy() for k, v in list(self.r.d.items()) + list(self.buf.items()) + list(self.r.o.items())}
        g.update({k: self.r.di[k].cpu().numpy().copy() for k in PRIOR + ("n_prior",)})
        g.update({"row_" + k: v.cpu().numpy().copy() for k, v in self.rows.items()})
        g["arc"] = [self.dev.h.get(b) for b in range(self.B)]
        g["obs"] = [self.obs.get(b) for b in range(self.B)]
        g["map_update"] = self.dev.status.cpu().numpy().copy()
        return g

    def same_state(self, g, b, w, a, st, where, base=None):
        t = br.pack(w)
        for k in br.TABLES:
            want = (self.r.host if base is None else base)[k][b].copy(); want[:len(t[k])] = t[k]       # rows from a new count on keep the bytes they had
            assert g[k][b, :len(t[k])].tobytes() == want[:len(t[k])].tobytes(), (where, b, k, "below the count")
            assert g[k][b].tobytes() == want.tobytes(), (where, b, k)
        assert (g["n_kf"][b], g["n_mp"][b], g["n_obs"][b]) == (len(t["kf_id"]), len(t["mp_id"]), len(t["obs_mp"])), (where, b)
        assert mr.same(g["arc"][b], a.arrays()) is None, (where, b, mr.same(g["arc"][b], a.arrays()))
        assert oa.same(g["obs"][b], st.arrays(a)) is None, (where, b, oa.same(g["obs"][b], st.arrays(a)))


def check_relink(x, g, items, want, seen=None, only=None, where0="re-link"):
    """everything the re-link of `items` must have left, against the walks `want`"""
    for b, (c, e) in enumerate(zip(items, want)):
        if only is not None and b not in only:
            continue
        where = (where0, c["spec"][0], c["cur_kf"])
        assert (g["plan_status"][b], g["stage_status"][b], g["be_status"][b], g["map_status"][b], g["map_update"][b], g["obs_status"][b]) == \
               (c["plan"]["status"], e["stage"]["status"], e["be"]["status"], e["map_status"], e["update_status"], e["obs_status"]), where
        x.same_state(g, b, e["w"], e["a"], e["st"], where)
        nm0 = len(c["w_before"].mps)
        assert g["new_row"][b, :nm0].tolist() == e["be"]["mp_new_row"].tolist() and (g["new_row"][b, nm0:] == SENT).all(), where
        rows = e["stage"]["rows"]
        n = len(rows)
        assert g["row_n"][b] == n, where
        if n:
            assert g["row_kf"][b, :n].tolist() == [r[0] for r in rows] and g["row_tag"][b, :n].tolist() == [r[3] for r in rows], where
            assert g["row_slot"][b, :n].tolist() == [r[7] for r in rows] and g["row_place"][b, :n].tolist() == [r[6] for r in rows], where
            assert g["row_root"][b, :n].tolist() == [r[5] for r in rows] and g["row_flags"][b, :n].tolist() == [r[4] for r in rows], where
            assert g["row_uv"][b, :n].tobytes() == np.array([(r[1], r[2]) for r in rows], np.float32).tobytes(), where
        n_mp = len(e["a"].mp_id)
        assert g["first_kf"][b, :n_mp].tolist() == e["first_kf"].tolist() and (g["first_kf"][b, n_mp:] == SENT).all(), where
        # the pending table of the current key-frame after both lists: what the plan left in place
        ref = rr.Store(F)
        pend = c["cur"].copy()
        hits = (ref.set_links(rr.moved_links(e["stage"]), pending_id=c["cur_kf"], pending=pend), ref.set_links(c["plan"]["links"], pending_id=c["cur_kf"], pending=pend))
        assert (g["n_set_rows"][b], g["n_set_plan"][b]) == hits and g["pend"][b].tobytes() == pend.tobytes(), where
        if e["be"]["status"] == rr.OK:
            assert g["pend"][b].tobytes() == c["plan"]["cur"].tobytes() and g["cur"][b].tobytes() == c["plan"]["cur"].tobytes(), where
        if seen is not None:
            seen["moved_rows"] += n; seen["relinks_done"] += e["be"]["status"] == rr.OK
            seen["appended_in_table"] += sum(1 for r in rows if r[5] in e["w"].mps)
            seen["appended_in_store"] += sum(1 for r in rows if r[5] not in e["w"].mps)


def run_batch(api, pkg, items, seen):
    x = Rows(api, pkg, items)
    want = [walk_relink(pkg.chain, c) for c in items]
    x.r.stream.wait_stream(x.torch.cuda.current_stream())
    x.relink()
    g = x.read()
    check_relink(x, g, items, want, seen)
    # ---- the device goes on: the next key-frame with the rows prior_rows_batch writes ----
    x.key_frame()
    g1, g = g, x.read()
    for b, (c, e) in enumerate(zip(items, want)):
        where = ("key-frame after", c["spec"][0], c["cur_kf"])
        ins = copy.deepcopy(c["next_insert"])
        w, a, st = e["w"], e["a"], e["st"]
        ps, priors = oa.prior_rows(st, [f[0] for f in ins.feats], sorted(w.mps), a, PRIOR_CAP)
        ins.priors = priors
        dis = g["dis"][b]
        rw = mi.insert_walk(w, ins, c["window"], 0.2, lambda pk, pn, row: dis[row])
        ms = mr.update(pkg.chain, a, mr.AFTER_INSERT, br.pack(w), rw["status"], outlier_ids=ins.outlier_ids, caps=ARCH_CAPS)
        so = oa.update(st, oa.AFTER_INSERT, br.pack(w), rw["status"], ms, a)
        assert (g["prior_status"][b], g["status"][b], g["map_update"][b], g["obs_status"][b]) == (ps, rw["status"], ms, so) and rw["status"] == mi.OK, where
        n = len(priors)                                                     # the arrays prior_rows_batch wrote are the walk's prior rows
        assert int(g["n_prior"][b]) == n, where
        assert g["prior_mp_id"][b, :n].tolist() == [q[0] for q in priors] and g["prior_kf_id"][b, :n].tolist() == [q[1] for q in priors], where
        assert g["prior_tag"][b, :n].tolist() == [q[3] for q in priors] and g["prior_flags"][b, :n].tolist() == [br.OUTLIER * bool(q[4]) for q in priors], where
        assert g["prior_uv"][b, :n].tobytes() == np.array([q[2] for q in priors], np.float32).reshape(-1, 2).tobytes(), where
        x.same_state(g, b, w, a, st, where, base=g1)
        back = {q[0] for q in priors} & c["touched"]
        flat, _, slot_mps = br.flatten(w)
        for j, mp in enumerate(slot_mps):
            if mp.id in back:
                assert flat["fixed"][j] == 1, (where, mp.id)               # the merged target returned as the fixed landmark src/backend.cpp:175-177 makes of it
                seen["returning_fixed_landmark"] += 1
    return x


def test_every_recorded_relink_and_the_key_frame_after_it(api, pkg, cases):
    seen = dict(moved_rows=0, relinks_done=0, appended_in_table=0, appended_in_store=0, returning_fixed_landmark=0, batches=0)
    for window in sorted({c["window"] for c in cases}):
        group = [c for c in cases if c["window"] == window]
        for i in range(0, len(group), 6):
            run_batch(api, pkg, group[i:i + 6], seen)
            seen["batches"] += 1
    print("\n%d items in %d batches: %s" % (len(cases), seen["batches"], seen))
    assert all(v > 0 for v in seen.values()), seen


def test_the_gap_without_the_row_calls_the_fused_point_stays_a_free_landmark(api, pkg, cases):
    """the parent's chain after a corrected loop (plan and states alone, no rows moved): the merged point is still in the back end's table and the next
    window optimises it as a free landmark; with the calls the table is the model's (the test above)"""
    c = next(c for c in cases if c["plan"]["status"] == rr.DONE and any(int(c["a_before"].mp_id[x]) in c["w_before"].mps for x, _ in c["plan"]["merge"]))
    x = Rows(api, pkg, [c])
    g = x.read()
    froms = [int(c["a_before"].mp_id[s]) for s, _ in c["plan"]["merge"] if int(c["a_before"].mp_id[s]) in c["w_before"].mps]
    flat, _, slot_mps = br.flatten(c["w_before"])
    free = [mp.id for j, mp in enumerate(slot_mps) if mp.id in froms and not flat["fixed"][j]]
    ids = g["mp_id"][0, :g["n_mp"][0]].tolist()
    assert free and all(i in ids for i in froms)                           # without the calls: rows of an erased point, a free landmark of the next solve
    e = walk_relink(pkg.chain, c)
    x.r.stream.wait_stream(x.torch.cuda.current_stream())
    x.relink()
    g = x.read()
    ids = g["mp_id"][0, :g["n_mp"][0]].tolist()
    assert not any(i in ids for i in froms) and ids == sorted(e["w"].mps)


def _needs(chain, c):
    e = walk_relink(chain, c, row_cap=1 << 20, obs_cap=1 << 20)
    return sum(len(rs) for _, rs in e["st"].live(e["a"])), len(br.pack(e["w"])["obs_mp"]), e


def test_capacity_one_row_below_is_refused_next_to_a_served_neighbour(api, pkg, cases):
    """row_cap and the back end's obs_cap one row below what an item's re-link needs: MYSLAM_ERR_CAPACITY from the stage, every byte of every table kept
    (no later call touches the item), while a neighbour that fits is served"""
    done = [c for c in cases if c["plan"]["status"] == rr.DONE]
    live_before = lambda c: sum(len(rs) for _, rs in c["st_before"].live(c["a_before"]))
    rows_before = lambda c: len(br.pack(c["w_before"])["obs_mp"])
    tried = 0
    for kind in ("row_cap", "obs_cap"):
        pick = None
        for c in done:
            need_live, need_rows, _ = _needs(pkg.chain, c)
            if kind == "row_cap" and need_live > live_before(c):
                pick = (c, need_live - 1, BE_CAPS)
            if kind == "obs_cap" and need_rows > rows_before(c) and need_rows - 1 >= max(FEAT_CAP, PRIOR_CAP):
                pick = (c, ROW_CAP, (BE_CAPS[0], BE_CAPS[1], need_rows - 1))
            if pick:
                break
        if pick is None:
            print("no recorded re-link grows the", kind, "side: the refusal is held by tests/test_relink_ref.py on the walk")
            continue
        c, row_cap, be_caps = pick
        small = next((d for d in done if d["window"] == c["window"] and d is not c and live_before(d) <= row_cap and _needs(pkg.chain, d)[0] <= row_cap
                      and _needs(pkg.chain, d)[1] <= be_caps[2] and rows_before(d) <= be_caps[2]), None)
        items = ([small] if small is not None else []) + [c]
        i = len(items) - 1
        x = Rows(api, pkg, items, row_cap=row_cap, be_caps=be_caps)
        before = x.read()
        x.r.stream.wait_stream(x.torch.cuda.current_stream())
        x.relink()
        g = x.read()
        assert g["stage_status"][i] == api.ERR_CAPACITY and g["be_status"][i] == api.ERR_CAPACITY, kind
        assert g["map_status"][i] == rr.MAP_SKIPPED and g["map_update"][i] == rr.MAP_SKIPPED and g["obs_status"][i] == rr.MAP_SKIPPED
        for k in br.TABLES + ("n_kf", "n_mp", "n_obs"):
            assert g[k][i].tobytes() == before[k][i].tobytes(), (kind, k)
        assert mr.same(g["arc"][i], before["arc"][i]) is None and oa.same(g["obs"][i], before["obs"][i]) is None and g["obs"][i]["error"] == 0
        if small is not None:
            assert g["stage_status"][0] == rr.DONE and g["be_status"][0] == 0
            e = walk_relink(pkg.chain, small, row_cap=row_cap, obs_cap=be_caps[2])
            x.same_state(g, 0, e["w"], e["a"], e["st"], kind)
        tried += 1
    assert tried >= 1


def test_call_level_errors_of_the_row_calls(api, pkg, cases):
    x = Rows(api, pkg, cases[:1])
    p = lambda k: x.buf[k].data_ptr()
    d = x.r.d

    def code(fn, *a):
        with pytest.raises(api.MyslamError) as e:
            fn(*a)
        return e.value.code

    assert code(x.rl.stage_batch, None, p("plan_status"), 1, p("stage_status")) == api.ERR_INVALID
    assert code(x.rl.stage_batch, x.obs, 0, 1, p("stage_status")) == code(x.rl.stage_batch, x.obs, p("plan_status"), 1, 0) == api.ERR_INVALID
    assert code(x.rl.stage_batch, x.obs, p("plan_status"), 2, p("stage_status")) == api.ERR_CAPACITY
    tabs = [d[k].data_ptr() for k in TABLE_ARGS]
    assert code(x.rl.backend_batch, None, *tabs, p("stage_status"), 1, p("new_row"), p("be_status")) == api.ERR_INVALID
    for i in range(13):
        assert code(x.rl.backend_batch, x.r.h, *(tabs[:i] + [0] + tabs[i + 1:]), p("stage_status"), 1, p("new_row"), p("be_status")) == api.ERR_INVALID, i
    assert code(x.rl.backend_batch, x.r.h, *tabs, p("stage_status"), 2, p("new_row"), p("be_status")) == api.ERR_CAPACITY
    reads = [d[k].data_ptr() for k in READ_ARGS]
    good = [x.obs] + reads + list(BE_CAPS) + [p("be_status"), x.dev.status.data_ptr(), 1, p("obs_status")]
    for i, v, want in ((0, None, api.ERR_INVALID), (1, 0, api.ERR_INVALID), (12, BE_CAPS[1] + 1, api.ERR_INVALID), (13, BE_CAPS[2] + 1, api.ERR_INVALID),
                       (14, 0, api.ERR_INVALID), (17, 0, api.ERR_INVALID), (16, 2, api.ERR_CAPACITY)):
        assert code(x.rl.obs_update_batch, *(good[:i] + [v] + good[i + 1:])) == want, i
    assert code(api.Relink.first_kf_batch, None, 1, p("first_kf")) == code(api.Relink.first_kf_batch, x.obs, 1, 0) == api.ERR_INVALID
    assert code(api.Relink.first_kf_batch, x.obs, 2, p("first_kf")) == api.ERR_CAPACITY
    other = api.MapArchive(1, 4, 4, ARCH_CAPS[2] + 1, BE_CAPS[1])           # a plan handle made for another archive's point_cap
    rl2 = api.Relink(other, 1, O, F, 64)
    assert code(rl2.stage_batch, x.obs, p("plan_status"), 1, p("stage_status")) == api.ERR_INVALID
    x.torch.cuda.synchronize()
    assert (x.read()["stage_status"] == SENT).all()


def _done(cases, pred=lambda c, e: True, chain=None):
    return [c for c in cases if c["plan"]["status"] == rr.DONE and len(c["plan"]["merge"]) >= 1 and pred(c, walk_relink(chain, c))]


def test_one_recording_of_the_whole_relink_replayed_on_a_second_loop_equals_the_walks(api, pkg, cases):
    """plan, stage, back end, map re-link, map update, observation update, first observers and both set_links recorded ONCE on the first items' buffers;
    other items' state goes into the same handles and buffers (these launches flip the mirror's and the pool's cursors and read counts on the
    device) and the recording is replayed: every table equals the walks, as after the eager calls"""
    window = max({c["window"] for c in cases}, key=lambda w: sum(c["window"] == w and c["plan"]["status"] == rr.DONE for c in cases))
    group = [c for c in cases if c["window"] == window]
    first, second = group[:3], group[3:6]
    assert len(second) == 3 and any(c["plan"]["status"] == rr.DONE for c in first) and any(c["plan"]["status"] == rr.DONE for c in second)
    x = Rows(api, pkg, first)
    sp = x.r.stream.cuda_stream
    x.r.stream.wait_stream(x.torch.cuda.current_stream())
    x.relink()                                                              # eager once, as the header's rules ask
    check_relink(x, x.read(), first, [walk_relink(pkg.chain, c) for c in first], where0="eager")
    x.load(first)
    g = api.StepGraph.record(sp, [], x.relink)
    assert g.node_count() == len(x.steps()) == 9
    g.launch(sp)
    check_relink(x, x.read(), first, [walk_relink(pkg.chain, c) for c in first], where0="recorded")
    x.load(second)
    g.launch(sp)
    check_relink(x, x.read(), second, [walk_relink(pkg.chain, c) for c in second], where0="replayed on a second loop")
    x.load(first)                                                           # and back: the cursors the first replay flipped do not matter
    g.launch(sp)
    check_relink(x, x.read(), first, [walk_relink(pkg.chain, c) for c in first], where0="replayed again")


def _kept(g, before, b, what):
    for k in br.TABLES + ("n_kf", "n_mp", "n_obs"):
        assert g[k][b].tobytes() == before[k][b].tobytes(), (what, k)
    assert mr.same(g["arc"][b], before["arc"][b]) is None, what


@pytest.mark.parametrize("fault", ["merge_slot", "merge_count", "target_not_standing", "table_count", "place_outside", "stale_staging"])
def test_a_faulty_item_of_the_row_calls_is_refused_by_status_between_served_neighbours(api, pkg, cases, fault):
    """a list or a count spoilt between two calls of item 1 of three: a merged slot = n_mp and a merge count beyond out_cap (the stage), a target that
    does not stand (the stage), a table count that is not the one the rows were staged for and a place outside what its point receives (the back
    end), a staging that is not of this mirror (the observation update: sticky).  The item keeps every byte of every table from that call on;
    its neighbours, the same calls around it, are served"""
    import torch
    in_table = lambda c, e: e["stage"]["rows"] and e["stage"]["rows"][0][5] in e["w"].mps
    good = _done(cases, in_table, pkg.chain)
    c = good[0]
    items = [c, c, next(d for d in good[1:] + good[:1] if d["window"] == c["window"])]
    x = Rows(api, pkg, items)
    want = [walk_relink(pkg.chain, d) for d in items]
    n_mp = len(c["a_before"].mp_id)
    snap = {}

    def spoil(name):
        if name == "plan":
            snap["before"] = x.read()
            if fault == "merge_slot":
                x.rows["merge"][1, 0, 0] = n_mp
            if fault == "merge_count":
                x.rows["n_merge"][1] = O + 1
            if fault == "target_not_standing":
                root = int(c["plan"]["target"][c["plan"]["merge"][0][0]])
                t = torch.as_tensor(DevArray(x.view.target, (3, ARCH_CAPS[2]), "<i4"), device="cuda")
                t[1, root] = -1
        if name == "stage" and fault in ("table_count", "place_outside"):
            if fault == "table_count":
                x.r.d["n_obs"][1] -= 1
            else:
                x.rows["place"][1, 0] = 10 ** 6
            torch.cuda.synchronize()
            snap["before"] = x.read()
        if name == "map_update" and fault == "stale_staging":
            x.rows["table_rows"][1] += 1
            torch.cuda.synchronize()
            snap["before"] = x.read()

    x.r.stream.wait_stream(torch.cuda.current_stream())
    x.relink(after=spoil)
    g = x.read()
    check_relink(x, g, items, want, only=(0, 2), where0=fault)
    before = snap["before"]
    if fault in ("merge_slot", "merge_count", "target_not_standing"):
        assert g["stage_status"][1] == api.ERR_INVALID and g["be_status"][1] == api.ERR_INVALID and g["row_n"][1] == 0
    if fault in ("table_count", "place_outside"):
        assert g["stage_status"][1] == rr.DONE and g["be_status"][1] == api.ERR_INVALID and (g["new_row"][1, :len(c["w_before"].mps)] == -1).all()
    if fault != "stale_staging":
        assert (g["map_status"][1], g["map_update"][1], g["obs_status"][1]) == (rr.MAP_SKIPPED,) * 3
        _kept(g, before, 1, fault)
        assert oa.same(g["obs"][1], before["obs"][1]) is None and g["obs"][1]["error"] == 0
    else:                                                                   # the back end and the map moved on; the observation archive refuses and stays refused
        assert (g["be_status"][1], g["map_status"][1], g["map_update"][1], g["obs_status"][1]) == (0, rr.MAP_UPDATED, mr.UPDATED, api.ERR_INVALID)
        _kept(g, before, 1, fault)
        assert g["obs"][1]["error"] == api.ERR_INVALID and all(np.asarray(g["obs"][1][k]).tobytes() == np.asarray(before["obs"][1][k]).tobytes() for k in oa.GET_FIELDS)
        assert (g["first_kf"][1, :n_mp] == -1).all()
        x.key_frame()                                                       # sticky: prior_rows and the next update answer the same error, the neighbours go on
        g2 = x.read()
        assert g2["prior_status"].tolist() == [0, api.ERR_INVALID, 0] and g2["n_prior"][1] == 0 and g2["obs_status"].tolist() == [0, api.ERR_INVALID, 0]


def test_stage_cap_one_row_below_is_refused_next_to_a_served_neighbour(api, pkg, cases):
    done = sorted(_done(cases, lambda c, e: len(e["stage"]["rows"]) >= 1, pkg.chain), key=lambda c: len(walk_relink(pkg.chain, c)["stage"]["rows"]))
    big = done[-1]
    small = next(d for d in done if d["window"] == big["window"] and d is not big)
    need = len(walk_relink(pkg.chain, big)["stage"]["rows"])
    assert len(walk_relink(pkg.chain, small)["stage"]["rows"]) < need
    for cap, status in ((need - 1, api.ERR_CAPACITY), (need, rr.DONE)):
        items = [small, big]
        x = Rows(api, pkg, items, stage_cap=cap)
        before = x.read()
        want = [walk_relink(pkg.chain, d, stage_cap=cap) for d in items]
        assert want[1]["stage"]["status"] == status and want[0]["stage"]["status"] == rr.DONE
        x.r.stream.wait_stream(x.torch.cuda.current_stream())
        x.relink()
        g = x.read()
        check_relink(x, g, items, want, where0="stage_cap %d" % cap)
        if status != rr.DONE:
            _kept(g, before, 1, "stage_cap")
            assert oa.same(g["obs"][1], before["obs"][1]) is None and g["obs"][1]["error"] == 0 and g["row_n"][1] == 0
