"""The re-link on the device (include/myslam_hip.h, RE-LINK): myslam_loop_relink_plan_batch, myslam_map_relink_batch, myslam_loop_store_set_links_batch and
myslam_tracker_relink_batch against the plain-Python rules of tests/relink_ref.py, on the re-links that tests/test_relink_ref.py holds against the object
model: the twelve histories as two batches of six items, every re-link of a history one call on its item.  After every call every byte the contract
names equals the rule: the plan's lists, target row, report and the current table, the archive's states, a stored and a pending table, the tracker's
features, landmarks and ids.  Then per-item refusals next to good neighbours, an item in another slot, one recording replayed on a second loop, and the
call-level errors.  Needs an MI355X."""
import numpy as np
import pytest

import map_insert_ref as mi
import relink_ref as rr
from test_whole_map_model import HISTORIES, K

pytestmark = pytest.mark.gpu

F, O = rr.FEAT_CAP, rr.OUT_CAP
SENT = -4242


class DevArray:
    """a device pointer of a handle's view as something torch can wrap (the CUDA array interface)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def runs(pkg):
    return [rr.run_history(pkg.chain, spec, K)[0] for spec in HISTORIES]


def skipped_case(like):
    """an item without a loop: the corrector skipped it; its arrays are a neighbour's, so that touching them would show"""
    return dict(like, correct_status=rr.CORRECT_SKIPPED, plan=rr.plan(like["pairs"], like["count"], like["outlier"], rr.CORRECT_SKIPPED, like["cur"], like["loop"],
                                                                     like["cur_kf"], like["mp_state"], len(like["mp_state"])), trk_out=like["trk_in"])


class World:
    """B items: a map archive, a plan handle, a loop store that holds each item's current key-frame, a tracker, and the call's buffers"""

    def __init__(self, api, B, P, lm_cap, stream=None, extra=1):
        import torch
        self.api, self.B, self.P, self.lm_cap, self.torch = api, B, P, lm_cap, torch
        sp = stream.cuda_stream if stream is not None else None
        self.stream = stream
        self.arc = api.MapArchive(B + extra, 4, 4, P, 8, stream=sp)
        self.rl = api.Relink(self.arc, B + extra, O, F, 8, stream=sp)
        self.trk = api.Tracker(B, 120, 160, F, lm_cap, K, stream=sp)
        self.store = api.LoopKeyFrameStore(B, 8, F, stream=sp)
        v = self.rl.view()
        assert (v.max_batch, v.out_cap, v.feat_cap, v.point_cap) == (B + extra, O, F, P)
        t = lambda ptr, shape, ty: torch.as_tensor(DevArray(ptr, shape, ty), device="cuda")
        n = B + extra
        self.out = dict(merge=t(v.merge, (n, O, 2), "<i4"), n_merge=t(v.n_merge, (n,), "<i4"), adopt=t(v.adopt, (n, O, 2), "<i4"), n_adopt=t(v.n_adopt, (n,), "<i4"),
                        target=t(v.target, (n, P), "<i4"), link_kf=t(v.link_kf_id, (n, F), "<i8"), link_tag=t(v.link_tag, (n, F), "<i4"),
                        link_slot=t(v.link_slot, (n, F), "<i4"), n_link=t(v.n_link, (n,), "<i4"), report=t(v.report, (n, 6), "<i4"))
        self.view = v
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.buf = dict(pairs=z((B, O, 2), torch.int32), counts=z((B,), torch.int32), outlier=z((B, O), torch.uint8), cstat=z((B,), torch.int32),
                        cur=z((B, F), torch.int32), loop=z((B, F), torch.int32), kf=z((B,), torch.int64), status=z((B,), torch.int32),
                        map_status=z((B,), torch.int32), pend=z((B, F), torch.int32), n_set=z((B,), torch.int32), n_set2=z((B,), torch.int32),
                        n_rel=z((B,), torch.int32), trk_status=z((B,), torch.int32))
        self.stored = False

    def fill(self, cases):
        """the inputs of one call: item b = cases[b]; the archive and the tracker of every item are loaded from its case"""
        torch, B = self.torch, self.B
        assert len(cases) == B
        host = dict(pairs=np.stack([c["pairs"] for c in cases]), counts=np.array([c["count"] for c in cases], np.int32), outlier=np.stack([c["outlier"] for c in cases]),
                    cstat=np.array([c["correct_status"] for c in cases], np.int32), cur=np.stack([c["cur"] for c in cases]), loop=np.stack([c["loop"] for c in cases]),
                    kf=np.array([c["cur_kf"] for c in cases], np.int64))
        for b, c in enumerate(cases):
            n = len(c["mp_id"])
            self.arc.load(b, [1], [mi.IDENT], [], [], np.zeros((0, 7)), c["mp_id"], c["mp_pos"], np.full(n, -1, np.int32), c["mp_state"])
            t = c["trk_in"]
            st = dict(xy=np.zeros((len(t["lm"]), 2), np.float32), lm=t["lm"], lm_pos=t["lm_pos"], lm_outlier=t["lm_outl"], ref_pose=mi.IDENT, ref_frame_id=t["ref_frame_id"],
                      last_rel=np.eye(4), rel_motion=np.eye(4), next_frame_id=t["next_frame_id"], status=1)
            self.trk.set_frame(b, st, image=np.zeros((120, 160), np.uint8))                      # (a stream's first hand-over needs an image)
            self.trk.set_ids(b, t["lm_id"], t["ref_kf_id"], t["ref_kf_id"] + 1, 10 ** 6)
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else torch.cuda.stream(torch.cuda.current_stream())
        with ctx:
            for k, v in host.items():
                self.buf[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
            self.buf["pend"].copy_(self.buf["cur"])
            for k in ("status", "map_status", "n_set", "n_set2", "n_rel", "trk_status"):
                self.buf[k].fill_(SENT)
            for k, v in self.out.items():
                v.fill_(SENT)
        torch.cuda.synchronize()
        return host

    def put_current(self, cases):
        """every item's current key-frame is stored once, with the table it has before the re-link (ids made ascending by the item)"""
        torch = self.torch
        ids = [1000 * b + 1 for b in range(self.B)]
        kps = torch.zeros((self.B, 8, 28), dtype=torch.uint8, device="cuda"); desc = torch.zeros((self.B, 8, 32), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(self.B, dtype=torch.int32, device="cuda"); nf = torch.full((self.B,), F, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.store.put_batch(ids, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), 0, self.buf["cur"].data_ptr(), nf.data_ptr())
        torch.cuda.synchronize()
        return np.array(ids, np.int64)

    def enqueue(self):
        p = lambda k: self.buf[k].data_ptr()
        v = self.view
        self.rl.plan_batch(p("pairs"), p("counts"), p("outlier"), p("cstat"), p("cur"), p("loop"), p("kf"), self.B, p("status"))
        self.arc.relink_batch(v.merge, v.n_merge, O, p("status"), self.B, p("map_status"))
        # the key-frame as a pending one: the table before the re-link, brought up to date by the link list
        self.store.set_links_batch(v.link_kf_id, v.link_tag, v.link_slot, v.n_link, F, self.B, p("kf"), p("pend"), p("n_set"))
        self.trk.relink_batch(v.link_kf_id, v.link_tag, v.link_slot, v.n_link, F, self.arc, p("n_rel"), p("trk_status"))

    def run(self):
        self.enqueue()
        self.torch.cuda.synchronize()

    def snapshot(self):
        g = {k: v.cpu().numpy().copy() for k, v in list(self.buf.items()) + list(self.out.items())}
        g["arc"] = [self.arc.get(b) for b in range(self.B)]
        g["trk"] = [(self.trk.get_frame(b), self.trk.get_ids(b)) for b in range(self.B)]
        return g

    def check(self, cases, host, g, tag=""):
        for b, c in enumerate(cases):
            p, w = c["plan"], (tag, b, c["spec"], c["cur_kf"])
            n_mp = len(c["mp_id"])
            assert g["status"][b] == p["status"], w
            assert g["n_merge"][b] == len(p["merge"]) and g["n_adopt"][b] == len(p["adopt"]) and g["n_link"][b] == len(p["links"]), w
            assert _same(g["merge"][b, :len(p["merge"])], np.array(p["merge"], np.int32).reshape(-1, 2)), w
            assert _same(g["adopt"][b, :len(p["adopt"])], np.array(p["adopt"], np.int32).reshape(-1, 2)), w
            assert (g["merge"][b, len(p["merge"]):] == SENT).all() and (g["adopt"][b, len(p["adopt"]):] == SENT).all(), w      # slots from a count on keep their bytes
            assert _same(g["target"][b, :n_mp], p["target"]) and (g["target"][b, n_mp:] == SENT).all(), w
            assert g["report"][b].tolist() == p["report"], w
            L = len(p["links"])
            want = np.array(p["links"], np.int64).reshape(-1, 3)
            assert _same(g["link_kf"][b, :L], want[:, 0]) and _same(g["link_tag"][b, :L], want[:, 1].astype(np.int32)) and _same(g["link_slot"][b, :L], want[:, 2].astype(np.int32)), w
            assert (g["link_tag"][b, L:] == SENT).all(), w
            assert _same(g["cur"][b], p["cur"]), w                          # the whole row, changed in place
            for k in ("pairs", "counts", "outlier", "cstat", "loop", "kf"):
                assert _same(g[k][b], host[k][b]), (w, k)                   # inputs keep their bytes
            done = p["status"] == rr.DONE
            assert g["map_status"][b] == (rr.MAP_UPDATED if done else rr.MAP_SKIPPED), w
            arc = g["arc"][b]
            assert _same(arc["mp_state"], c["state_after"] if done else c["mp_state"]) and _same(arc["mp_id"], c["mp_id"]) and _same(arc["mp_pos"], c["mp_pos"]), w
            assert _same(g["pend"][b], p["cur"]) and g["n_set"][b] == L, w  # a pending table + the link list = the plan's table
            st, ids = g["trk"][b]
            t = c["trk_out"]
            assert g["trk_status"][b] == rr.OK and g["n_rel"][b] == L, w
            assert _same(st["lm"], t["lm"]) and _same(ids["landmark_id"], t["lm_id"]) and _same(st["lm_pos"], t["lm_pos"]) and _same(st["lm_outlier"], t["lm_outl"]), w
            assert ids["ref_kf_id"] == t["ref_kf_id"] and ids["next_mp_id"] == 10 ** 6 and st["next_frame_id"] == t["next_frame_id"] and st["frozen"] == 0, w


def _batches(runs):
    return [runs[:6], runs[6:]]


@pytest.mark.parametrize("half", [0, 1])
def test_histories_on_the_device_equal_the_walk_after_every_relink(api, runs, half):
    """and THE GAP ITSELF: before the calls the merged point of a corrected loop is still alive in myslam_map (state 0: the back end would go on
    optimising it as a free landmark and every later key-frame would insert rows for it); with the calls its state is the model's"""
    items = _batches(runs)[half]
    B = len(items)
    P = max(len(c["mp_id"]) for cs in items for c in cs) + 5
    w = World(api, B, P, max(c["lm_cap"] for cs in items for c in cs))
    steps = max(len(cs) for cs in items)
    n_done = n_gap = 0
    for r in range(steps):
        like = next(cs[r] for cs in items if r < len(cs))
        cases = [cs[r] if r < len(cs) else skipped_case(like) for cs in items]
        host = w.fill(cases)
        for b, c in enumerate(cases):                                       # without the calls: every point the model merged away is still alive on the device
            froms = [a for a, _ in c["plan"]["merge"]]
            if froms:
                assert (w.arc.get(b)["mp_state"][froms] != 2).all() and (c["state_after"][froms] == 2).all()
                n_gap += len(froms)
        w.run()
        g = w.snapshot()
        w.check(cases, host, g, tag="step %d" % r)
        assert (g["n_merge"][B:] == SENT).all() and (g["target"][B:] == SENT).all() and (g["report"][B:] == SENT).all()      # items beyond the batch keep their bytes
        n_done += sum(c["plan"]["status"] == rr.DONE for c in cases)
    print("\nbatch %d: %d steps, %d re-links done, %d merged points that were alive without the calls" % (half, steps, n_done, n_gap))
    assert n_done >= B and n_gap > 0


def _one(runs, pred):
    return next(c for cs in runs for c in cs if c["plan"]["status"] == rr.DONE and pred(c))


def test_a_stored_key_frame_follows_the_link_list(api, runs):
    """the current key-frame is held by the store (no pending table): set_links_batch brings its stored table to the plan's; ids not held, tags out of range
    and slots below -1 are ignored"""
    import torch
    cases = [_one(runs, lambda c: len(c["plan"]["links"]) >= 3), _one(runs, lambda c: any(s < 0 for _, _, s in c["plan"]["links"]))]
    w = World(api, 2, max(len(c["mp_id"]) for c in cases) + 5, max(c["lm_cap"] for c in cases))
    w.fill(cases)
    ids = w.put_current(cases)
    ref = rr.Store(F)
    lists = []
    for b, c in enumerate(cases):
        ref.put(int(ids[b]), c["cur"], F)
        lists.append([(int(ids[b]), f, s) for _, f, s in c["plan"]["links"]] + [(int(ids[b]) + 5, 0, 1), (int(ids[b]), F, 1), (int(ids[b]), 0, -2), (-1, 0, 1)])
    L = max(len(l) for l in lists) + 2
    kf = np.full((2, L), -5, np.int64); tag = np.full((2, L), -6, np.int32); slot = np.full((2, L), -7, np.int32)
    for b, l in enumerate(lists):
        for j, (i, f, s) in enumerate(l):
            kf[b, j], tag[b, j], slot[b, j] = i, f, s
    n = np.array([len(lists[0]), L + 9], np.int32)                          # above list_cap: reads as list_cap (the spare entries name nothing)
    d = [torch.from_numpy(x).cuda() for x in (kf, tag, slot, n)]
    d_n = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    w.store.set_links_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, 2, None, None, d_n.data_ptr())
    torch.cuda.synchronize()
    want = [ref.set_links(lists[b] + [(-5, -6, -7)] * L, n=n[b], list_cap=L) for b in range(2)]
    assert d_n.cpu().numpy().tolist() == want == [len(c["plan"]["links"]) for c in cases]
    # gather the two key-frames: detect_batch with a threshold every score passes
    o = dict(desc=torch.zeros((2, 8, 32), dtype=torch.uint8, device="cuda"), n=torch.zeros(2, dtype=torch.int32, device="cuda"),
             pyr=torch.zeros((2, 8, 28), dtype=torch.uint8, device="cuda"), lm=torch.full((2, F), SENT, dtype=torch.int32, device="cuda"),
             slot=torch.zeros(2, dtype=torch.int32, device="cuda"), st=torch.zeros(2, dtype=torch.int32, device="cuda"))
    q = [torch.from_numpy(ids.astype(np.uint64).view(np.int64)).cuda(), torch.ones(2, dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    w.store.detect_batch(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), 2, o["desc"].data_ptr(), o["n"].data_ptr(), o["pyr"].data_ptr(), o["lm"].data_ptr(),
                         o["slot"].data_ptr(), o["st"].data_ptr(), thr_high=0.5)
    torch.cuda.synchronize()
    assert o["st"].cpu().numpy().tolist() == [0, 0]
    for b, c in enumerate(cases):
        assert _same(o["lm"].cpu().numpy()[b], c["plan"]["cur"]) and _same(ref.gather(int(ids[b])), c["plan"]["cur"]), b
    for bad in ((0, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, 2), (d[0].data_ptr(), d[1].data_ptr(), 0, d[3].data_ptr(), L, 2),
                (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, 2), (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, 0),
                (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, 2, d[0].data_ptr(), None)):
        with pytest.raises(api.MyslamError) as e:
            w.store.set_links_batch(*bad)
        assert e.value.code == api.ERR_INVALID


def test_refused_items_keep_every_byte_next_to_good_neighbours(api, runs):
    """a bad slot in either table, a bad feature id, a bad count, a bad key-frame id: refused by status before any access;
    the archive's states, the tables and the tracker of such an item are untouched, and its neighbours (the same good item on both sides) are served"""
    good = _one(runs, lambda c: len(c["plan"]["merge"]) >= 2 and len(c["plan"]["adopt"]) >= 1)
    n_mp = len(good["mp_id"])
    walked = [i for i in range(good["count"]) if not good["outlier"][i]]
    cf, lf = (int(v) for v in good["pairs"][walked[-1]])

    def broken(**kw):
        c = dict(good)
        for k, v in kw.items():
            if k in ("cur", "loop", "pairs"):
                a = c[k].copy(); a[v[0]] = v[1]; c[k] = a
            else:
                c[k] = v
        c["plan"] = rr.plan(c["pairs"], c["count"], c["outlier"], c["correct_status"], c["cur"], c["loop"], c["cur_kf"], c["mp_state"], n_mp, point_cap=n_mp + 5)
        assert c["plan"]["status"] == rr.INVALID and _same(c["plan"]["cur"], c["cur"])
        c["trk_out"] = c["trk_in"]
        return c

    bad = [broken(cur=(cf, n_mp)), broken(loop=(lf, n_mp)), broken(cur=(cf, -2)), broken(pairs=(walked[0], (F, lf))), broken(pairs=(walked[0], (cf, -1))),
           broken(count=-1), broken(count=O + 1), broken(cur_kf=-3)]
    for k in range(0, len(bad), 2):
        cases = [good, bad[k], good, bad[k + 1], good]
        w = World(api, 5, n_mp + 5, good["lm_cap"])
        host = w.fill(cases)
        w.run()
        w.check(cases, host, w.snapshot(), tag="faults %d" % k)


def test_map_relink_and_tracker_refuse_by_status(api, runs):
    """hand-made lists: a merge list with a slot out of range or a bad count leaves every state; the tracker refuses a slot out of range and a full
    landmark table (one slot below what the list needs) with every byte kept, and serves the same list with one slot more"""
    import torch
    c = _one(runs, lambda c: c["trk_out"]["lm_id"].size > c["trk_in"]["lm_id"].size and len(c["plan"]["merge"]) >= 1)
    n_mp = len(c["mp_id"])
    need = len(c["trk_out"]["lm_id"])
    for lm_cap, want in ((need - 1, api.ERR_CAPACITY), (need, rr.OK)):
        w = World(api, 3, n_mp + 5, lm_cap)
        cases = [c, c, c]
        w.fill(cases)
        p = lambda k: w.buf[k].data_ptr()
        w.rl.plan_batch(p("pairs"), p("counts"), p("outlier"), p("cstat"), p("cur"), p("loop"), p("kf"), 3, p("status"))
        torch.cuda.synchronize()
        # item 1's lists are spoilt by hand: a from-slot = n_mp in the merge list, a link slot = n_mp
        w.out["merge"][1, 0, 0] = n_mp
        w.out["link_slot"][1, 0] = n_mp
        w.out["n_merge"][2] = O + 1
        torch.cuda.synchronize()
        v = w.view
        w.arc.relink_batch(v.merge, v.n_merge, O, p("status"), 3, p("map_status"))
        w.trk.relink_batch(v.link_kf_id, v.link_tag, v.link_slot, v.n_link, F, w.arc, p("n_rel"), p("trk_status"))
        torch.cuda.synchronize()
        g = w.snapshot()
        assert g["map_status"].tolist() == [rr.MAP_UPDATED, api.ERR_INVALID, api.ERR_INVALID]
        assert _same(g["arc"][0]["mp_state"], c["state_after"]) and _same(g["arc"][1]["mp_state"], c["mp_state"]) and _same(g["arc"][2]["mp_state"], c["mp_state"])
        assert g["trk_status"].tolist() == [want, api.ERR_INVALID, want]
        for b in range(3):
            st, ids = g["trk"][b]
            t = c["trk_out"] if (b != 1 and want == rr.OK) else c["trk_in"]
            assert _same(st["lm"], t["lm"]) and _same(ids["landmark_id"], t["lm_id"]) and _same(st["lm_pos"], t["lm_pos"]) and _same(st["lm_outlier"], t["lm_outl"]), (lm_cap, b)
            assert g["n_rel"][b] == (len(c["plan"]["links"]) if (b != 1 and want == rr.OK) else 0)
    # a stream that has stepped since its key-frame, and one without valid ids, keep every byte
    w = World(api, 2, n_mp + 5, need)
    stepped = dict(c, trk_in=dict(c["trk_in"], next_frame_id=c["trk_in"]["next_frame_id"] + 1))
    stepped["trk_out"] = stepped["trk_in"]
    host = w.fill([stepped, c])
    w.run()
    g = w.snapshot()
    assert g["n_rel"].tolist() == [0, len(c["plan"]["links"])] and g["trk_status"].tolist() == [0, 0]
    w.check([stepped, c], host, dict(g, n_rel=np.array([len(c["plan"]["links"])] * 2, np.int32)))


def test_an_item_in_another_slot_gives_the_same_bytes(api, runs):
    a = _one(runs, lambda c: len(c["plan"]["merge"]) >= 2 and len(c["plan"]["links"]) >= 3)
    others = [c for cs in runs for c in cs if c is not a and c["plan"]["status"] == rr.DONE][:3]
    P = max(len(c["mp_id"]) for c in [a] + others) + 5
    lm_cap = max(c["lm_cap"] for c in [a] + others)
    snaps = []
    for cases, slot in (([a, others[0], others[1]], 0), ([others[2], others[1], a], 2)):
        w = World(api, 3, P, lm_cap)
        host = w.fill(cases)
        w.run()
        g = w.snapshot()
        w.check(cases, host, g)
        snaps.append({k: (v[slot] if k not in ("arc", "trk") else v[slot]) for k, v in g.items()})
    x, y = snaps
    for k in x:
        if k == "arc":
            assert all(_same(x[k][f], y[k][f]) for f in x[k]), k
        elif k == "trk":
            assert all(_same(x[k][0][f], y[k][0][f]) for f in x[k][0]) and all(_same(x[k][1][f], y[k][1][f]) for f in x[k][1]), k
        else:
            assert _same(x[k], y[k]), k


def test_one_recording_replayed_on_a_second_loop_equals_eager(api, runs):
    """plan + map re-link + set_links + tracker re-link recorded once on the first loop's buffers; the second loop's inputs go into the same buffers and
    the recording is replayed: every output equals the eager calls'"""
    import torch
    item = max(runs, key=lambda cs: sum(c["plan"]["status"] == rr.DONE for c in cs))
    loops = [c for c in item if c["plan"]["status"] == rr.DONE][:2]
    other = _one(runs, lambda c: c["spec"] != loops[0]["spec"])
    assert len(loops) == 2
    P = max(len(c["mp_id"]) for c in loops + [other]) + 5
    lm_cap = max(c["lm_cap"] for c in loops + [other])
    got = {}
    for recorded in (False, True):
        stream = torch.cuda.Stream()
        w = World(api, 2, P, lm_cap, stream=stream)
        assert w.rl.launches_per_plan() == 1
        w.fill([loops[0], other])
        if recorded:
            w.run()                                                         # eager once, as the header's rules ask, then from the same inputs again
            w.fill([loops[0], other])
            g = api.StepGraph.record(stream.cuda_stream, [], w.enqueue)
            assert g.node_count() == 4
            g.launch(stream.cuda_stream)
        else:
            w.enqueue()
        stream.synchronize()
        first = w.snapshot()
        host = w.fill([loops[1], skipped_case(other)])
        if recorded:
            g.launch(stream.cuda_stream)
        else:
            w.enqueue()
        stream.synchronize()
        second = w.snapshot()
        w.check([loops[1], skipped_case(other)], host, second, tag="recorded" if recorded else "eager")
        got[recorded] = (first, second)
    for a, b in zip(got[False], got[True]):
        for k in a:
            if k in ("arc", "trk"):
                continue
            assert _same(a[k], b[k]), k
        for x, y in zip(a["arc"], b["arc"]):
            assert all(_same(x[f], y[f]) for f in x)
        for (xs, xi), (ys, yi) in zip(a["trk"], b["trk"]):
            assert all(_same(xs[f], ys[f]) for f in xs) and all(_same(xi[f], yi[f]) for f in xi)


def test_call_level_errors(api, runs):
    import torch
    c = runs[0][0]
    w = World(api, 2, len(c["mp_id"]) + 5, c["lm_cap"])
    w.fill([c, c])
    p = lambda k: w.buf[k].data_ptr()
    v = w.view
    args = [p("pairs"), p("counts"), p("outlier"), p("cstat"), p("cur"), p("loop"), p("kf"), 2, p("status")]
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        a = list(args); a[i] = 0
        with pytest.raises(api.MyslamError) as e:
            w.rl.plan_batch(*a)
        assert e.value.code == api.ERR_INVALID, i
    for batch, code in ((-1, api.ERR_INVALID), (4, api.ERR_CAPACITY)):
        a = list(args); a[7] = batch
        with pytest.raises(api.MyslamError) as e:
            w.rl.plan_batch(*a)
        assert e.value.code == code
    a = list(args); a[7] = 0
    w.rl.plan_batch(*a)                                                     # an empty batch enqueues nothing
    margs = [v.merge, v.n_merge, O, p("status"), 2, p("map_status")]
    for i, val, code in ((0, 0, api.ERR_INVALID), (1, 0, api.ERR_INVALID), (2, 0, api.ERR_INVALID), (3, 0, api.ERR_INVALID), (5, 0, api.ERR_INVALID),
                         (4, -1, api.ERR_INVALID), (4, 4, api.ERR_CAPACITY)):
        a = list(margs); a[i] = val
        with pytest.raises(api.MyslamError) as e:
            w.arc.relink_batch(*a)
        assert e.value.code == code, i
    targs = [v.link_kf_id, v.link_tag, v.link_slot, v.n_link, F, w.arc, p("n_rel"), p("trk_status")]
    for i, val in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, None), (7, 0)):
        a = list(targs); a[i] = val
        with pytest.raises(api.MyslamError) as e:
            w.trk.relink_batch(*a)
        assert e.value.code == api.ERR_INVALID, i
    tiny = api.MapArchive(1, 4, 4, 8, 8)                                    # fewer items than the tracker has streams
    with pytest.raises(api.MyslamError) as e:
        w.trk.relink_batch(*(targs[:5] + [tiny] + targs[6:]))
    assert e.value.code == api.ERR_INVALID
    for bad, code in (((3, O, F, 8), api.ERR_INVALID), ((0, O, F, 8), api.ERR_INVALID), ((1, 0, F, 8), api.ERR_INVALID), ((1, O, 0, 8), api.ERR_INVALID),
                      ((1, O, F, 0), api.ERR_INVALID), ((1, 4097, F, 8), api.ERR_CAPACITY), ((1, O, 65537, 8), api.ERR_CAPACITY)):
        with pytest.raises(api.MyslamError) as e:
            api.Relink(tiny, *bad)
        assert e.value.code == code, bad
    torch.cuda.synchronize()
    g = w.snapshot()
    assert (g["status"] == SENT).all() and _same(g["cur"][0], c["cur"])    # nothing was enqueued by any refused call
