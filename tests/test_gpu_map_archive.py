"""myslam_map_update_batch (csrc/map_archive.hip, k_map_update): the whole map of every stream kept on the device from the back end's tables.  After every
call the archive of every item (api.MapArchive.get: all thirteen arrays, the snapshot and the window record included) must equal
tests/map_archive_ref.py's walk byte for byte, the walk being fed the tables, statuses and reports the device itself produced; the statuses must be the
walk's.  Sequences of insert -> update -> optimise -> update on synthetic maps (ids with gaps, key-frames leaving the window, points erased by the
optimiser, points leaving alive, outlier ids inside and outside the active table), hand-made sizes around the 256-thread workgroup, every refusal with
its untouched bytes, slot independence, load / get, and a recorded step."""
import numpy as np
import pytest

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
from test_gpu_map_insert import OUT_FILL, TABLE_ARGS, Run, next_keyframe

pytestmark = pytest.mark.gpu

MAP_TABLES = ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "n_mp", "obs_mp", "obs_kf", "obs_flags", "n_obs")
STATUS_FILL = -91


def tables_of(d, b):
    """item b of downloaded back-end tables, cut to its counts: what the walk reads"""
    nk, nm, no = int(d["n_kf"][b]), int(d["n_mp"][b]), int(d["n_obs"][b])
    return dict(kf_id=d["kf_id"][b, :nk], kf_pose=d["kf_pose"][b, :nk], mp_id=d["mp_id"][b, :nm], mp_pos=d["mp_pos"][b, :nm], obs_mp=d["obs_mp"][b, :no],
                obs_kf=d["obs_kf"][b, :no], obs_flags=d["obs_flags"][b, :no])


class Dev:
    """an archive handle next to back-end tables held as torch tensors `d` (name -> tensor, the layout of backend_ref.pack_batch)"""

    def __init__(self, api, B, caps, be_caps, stream):
        import torch
        self.torch, self.api, self.B, self.caps, self.be_caps, self.stream = torch, api, B, caps, be_caps, stream
        self.h = api.MapArchive(B, caps[0], caps[1], caps[2], be_caps[1], stream=stream.cuda_stream)
        self.status = torch.full((B,), STATUS_FILL, dtype=torch.int32, device="cuda")

    def update(self, mode, d, be_status, outlier=None, n_outlier=None, outlier_cap=0, report=None, batch=None):
        p = lambda t: t.data_ptr() if t is not None else None
        self.h.update_batch(mode, p(d["kf_id"]), p(d["kf_pose"]), p(d["n_kf"]), self.be_caps[0], p(d["mp_id"]), p(d["mp_pos"]), p(d["n_mp"]), self.be_caps[1],
                            p(d["obs_mp"]), p(d["obs_kf"]), p(d["obs_flags"]), p(d["n_obs"]), self.be_caps[2], p(be_status), p(outlier), p(n_outlier),
                            outlier_cap, p(report), self.B if batch is None else batch, p(self.status))

    def read(self):
        self.stream.synchronize()
        return [self.h.get(b) for b in range(self.B)], self.status.cpu().numpy().copy()


def walk_and_compare(chain, dev, walks, mode, d_host, be_status, outl=None, report=None, caps=None):
    """advance every item's walk with what the device's back end left, then the device's archive and status must be the walk's"""
    got, st = dev.read()
    for b, a in enumerate(walks):
        ids = () if outl is None else outl[0][b, :int(outl[1][b])]
        rep = None if report is None else report[b]
        want = mr.update(chain, a, mode, tables_of(d_host, b), int(be_status[b]), outlier_ids=ids, mp_report=rep, caps=caps or dev.caps)
        assert st[b] == want, (b, st[b], want)
        assert mr.same(got[b], a.arrays()) is None, (b, mr.same(got[b], a.arrays()))
    return st


def test_sequences_of_insert_update_optimise_update(api, pkg, synth):
    """8 key-frames on 3 maps at a window of 4: the first update archives a whole table (several key-frames at once, an edge between each two), then
    key-frames leave the window, the optimiser erases points, points leave alive and come back, outlier ids name points inside the table, points that
    left it and ids nobody knows"""
    import torch
    made = [br.make_map(synth, s, n_kf=4, n_mp=60) for s in (0x310, 0x311, 0x312)]
    cur, K = [x[0].clone() for x in made], made[0][1]
    be_caps, feat_cap, window, B = (8, 160, 1600), 64, 4, 3
    rng = np.random.default_rng(0xA3C1)
    first = [next_keyframe(pkg.chain, m, K, 0, rng) for m in cur]
    r = Run(api, cur, first, window, 0.2, caps=(be_caps, feat_cap, 2, 6))
    dev = Dev(api, B, (32, 31, 400), be_caps, r.stream)
    walks = [mr.Archive() for _ in range(B)]
    full = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    oo = dict(obs_report=full((B, be_caps[2]), torch.uint8), mp_report=full((B, be_caps[1]), torch.uint8), new_outlier=full((B, be_caps[1]), torch.int32),
              n_new=full((B,), torch.int32), obs_chi2=full((B, be_caps[2]), torch.float64), rounds=full((B,), torch.int32), n_out=full((B,), torch.int32),
              status=full((B,), torch.int32))
    r.stream.wait_stream(torch.cuda.current_stream())
    seen = dict(erased=0, left=0, promoted=0, gone=0, back=0)
    for step in range(8):
        inss = first if step == 0 else [next_keyframe(pkg.chain, mr_map(tables_of(host, b)), K, step, rng) for b in range(B)]
        for b, ins in enumerate(inss):
            a = walks[b]
            table = set(int(v) for v in tables_of(host, b)["mp_id"]) if step else set()
            if a.mp_id:                                                     # ids come from a counter: a new one is above every id the map ever held
                ins.feats = [f for f in ins.feats if f[0] < 0 or f[0] in table or f[0] > a.mp_id[-1]]
            named = set(int(f[0]) for f in ins.feats)
            away = [(i, p) for i, p, s in zip(a.mp_id, a.mp_pos, a.mp_state) if s == 0 and i not in named and i not in table]
            if len(away) > 2:                                               # a point that left the table comes back: it is found, not appended
                ins.feats.append((away[2][0], tuple(away[2][1]), (33.0, 44.0), 777000 + step, False)); seen["back"] += 1
            # outlier ids outside the active table: points that left it, an id nobody knows
            ins.outlier_ids = list(ins.outlier_ids) + [i for i, _ in away[:2]] + [987654]
        r.inp = mi.pack_inputs(inss, feat_cap, 2, 6)
        with torch.cuda.stream(r.stream):
            for k, v in r.inp.items():
                r.di[k].copy_(torch.from_numpy(v))
            for k, v in r.o.items():
                v.fill_(OUT_FILL[k])
        r.enqueue()
        dev.update(mr.AFTER_INSERT, r.d, r.o["status"], r.di["outlier_mp_id"], r.di["n_outlier"], 6)
        out = r.results()
        assert (out["status"] == 0).all()
        walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, out, out["status"], outl=(r.inp["outlier_mp_id"], r.inp["n_outlier"]))
        seen["gone"] += sum(int((a.arrays()["mp_gone_kf"] >= 0).sum()) for a in walks)
        r.h.optimize_batch(*[r.d[k].data_ptr() for k in TABLE_ARGS], B, K,
                           *[oo[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2", "rounds", "n_out", "status")])
        dev.update(mr.AFTER_OPTIMIZE, r.d, oo["status"], report=oo["mp_report"])
        r.stream.synchronize()
        host = {k: v.cpu().numpy() for k, v in r.d.items()}
        rep, ost = oo["mp_report"].cpu().numpy(), oo["status"].cpu().numpy()
        assert (ost == br.DONE).all()
        pre = [(list(a.mp_state), len(a.snapshot)) for a in walks]
        walk_and_compare(pkg.chain, dev, walks, mr.AFTER_OPTIMIZE, host, ost, report=rep)
        for b, a in enumerate(walks):
            seen["left"] += int((rep[b, :pre[b][1]] == 1).sum())
            seen["erased"] += sum(1 for x, y in zip(pre[b][0], a.mp_state) if x == 0 and y == 2)
            seen["promoted"] += sum(1 for x, y in zip(pre[b][0], a.mp_state) if x == 1 and y == 2)
    assert all(len(a.kf_id) >= 10 and len(a.edge_v0) == len(a.kf_id) - 1 for a in walks)
    print("paths met:", seen)
    assert all(v > 0 for v in seen.values()), seen


def mr_map(t):
    """the little of a backend_ref.Map that next_keyframe reads, from downloaded tables"""
    m = br.Map()
    for k, p in zip(t["kf_id"], t["kf_pose"]):
        m.kfs[int(k)] = np.array(p, float)
    for i, p in zip(t["mp_id"], t["mp_pos"]):
        m.mps[int(i)] = br.MapPoint(int(i), p)
    return m


def hand_tables(maps, be_caps):
    import torch
    host = br.pack_batch(maps, *be_caps)
    return host, {k: torch.from_numpy(host[k].copy()).cuda() for k in MAP_TABLES}


@pytest.mark.parametrize("n_mp", [0, 1, 255, 256, 257, 300])
def test_map_point_counts_around_the_workgroup(api, pkg, n_mp):
    """one AFTER_INSERT update of a hand-made table with n_mp points (300 = backend_mp_cap), next to a neighbour of another size; then a second update
    after the table lost rows and gained ids: found rows, appended rows, the snapshot"""
    import torch
    be_caps = (4, 300, 700)
    kf = [3, 5, 8]
    maps = [mi.small_map(kf, [mi.shifted(1.0 + i) for i in range(3)], n_mp, first_mp_id=100, mp_step=3, seed=n_mp), mi.small_map(kf, [mi.shifted(2.0 + i) for i in range(3)], 7, seed=1)]
    host, d = hand_tables(maps, be_caps)
    stream = torch.cuda.Stream(); stream.wait_stream(torch.cuda.current_stream())
    dev = Dev(api, 2, (6, 5, 400), be_caps, stream)
    walks = [mr.Archive(), mr.Archive()]
    zero = torch.zeros(2, dtype=torch.int32, device="cuda")
    dev.update(mr.AFTER_INSERT, d, zero)
    st = walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, host, [0, 0])
    assert (st == mr.UPDATED).all() and len(walks[0].mp_id) == n_mp and len(walks[0].edge_v0) == 2
    # every third point leaves the table, one key-frame leaves, a new key-frame and new ids above the archive's last arrive
    m2 = mi.small_map([5, 8, 11], [mi.shifted(2.5 + i) for i in range(3)], n_mp, first_mp_id=100, mp_step=3, seed=n_mp)
    for j, mid in enumerate(sorted(m2.mps)):
        if j % 3 == 1:
            del m2.mps[mid]
    for j in range(min(n_mp, 40)):
        m2.mps[100000 + 5 * j] = br.MapPoint(100000 + 5 * j, (j, 1.0, 9.0))
        o = br.Obs(11, 1.0, 2.0, False, j); m2.mps[100000 + 5 * j].obs.append(o); m2.mps[100000 + 5 * j].active_obs.append(o)
    host2, d2 = hand_tables([m2, maps[1]], be_caps)
    dev.update(mr.AFTER_INSERT, d2, zero)
    st = walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, host2, [0, 0])
    assert (st == mr.UPDATED).all() and walks[0].kf_id == [3, 5, 8, 11] and len(walks[0].mp_id) == n_mp + min(n_mp, 40)
    if n_mp >= 255:
        assert (walks[0].arrays()["mp_gone_kf"] == 0).sum() > 50             # key-frame 3 left the window: the points it observed remember it


def test_refusals_keep_every_byte(api, pkg):
    """a refused insert and an EMPTY optimise (state 1 stays), caps met exactly and exceeded by one, an unarchived id below the archive's last"""
    import torch
    be_caps = (4, 40, 200)
    big = mi.small_map([3, 5, 8, 9], [mi.shifted(1.0 + i) for i in range(4)], 10)
    small = mi.small_map([3, 5, 8], [mi.shifted(1.0 + i) for i in range(3)], 9)
    host, d = hand_tables([big, small], be_caps)
    stream = torch.cuda.Stream(); stream.wait_stream(torch.cuda.current_stream())
    zero = torch.zeros(2, dtype=torch.int32, device="cuda")
    for caps in ((3, 8, 20), (8, 2, 20), (8, 8, 9)):                        # item 0 exceeds the cap by one, item 1 meets it exactly
        dev = Dev(api, 2, caps, be_caps, stream)
        walks = [mr.Archive(), mr.Archive()]
        dev.update(mr.AFTER_INSERT, d, zero)
        st = walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, host, [0, 0])
        assert list(st) == [mr.CAPACITY, mr.UPDATED] and walks[0].kf_id == [] and walks[0].mp_id == []
        assert (len(walks[1].kf_id), len(walks[1].edge_v0), len(walks[1].mp_id)) == (3, 2, 9)
    dev = Dev(api, 2, (4, 3, 10), be_caps, stream)                          # item 0 meets all three exactly
    walks = [mr.Archive(), mr.Archive()]
    dev.update(mr.AFTER_INSERT, d, zero)
    assert list(walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, host, [0, 0])) == [mr.UPDATED, mr.UPDATED]
    # a refused insert (status -1) and an optimise that found nothing to do (EMPTY): untouched, the outlier-list point keeps state 1
    a = walks[0]
    a.mp_state[2] = 1
    arr = a.arrays()
    dev.h.load(0, *[arr[k] for k in ("kf_id", "kf_pose", "edge_v0", "edge_v1", "meas", "mp_id", "mp_pos", "mp_first_kf", "mp_state", "snapshot", "mp_gone_kf",
                                     "mp_win_mask", "win_kf")])
    report = torch.full((2, be_caps[1]), 2, dtype=torch.uint8, device="cuda")
    for mode, status in ((mr.AFTER_INSERT, [-1, 0]), (mr.AFTER_OPTIMIZE, [br.EMPTY, -3]), (mr.AFTER_OPTIMIZE, [-1, br.EMPTY])):
        dev.update(mode, d, torch.tensor(status, dtype=torch.int32, device="cuda"), report=report)
        st = walk_and_compare(pkg.chain, dev, walks, mode, host, status, report=report.cpu().numpy())
        assert st[0] == mr.SKIPPED and walks[0].mp_state[2] == 1
    # an id the archive never saw, below its last id
    odd = big.clone(); odd.mps[101] = br.MapPoint(101, (0.0, 0.0, 5.0)); o = br.Obs(3, 1.0, 1.0, False, 1); odd.mps[101].obs.append(o); odd.mps[101].active_obs.append(o)
    host3, d3 = hand_tables([odd, small], be_caps)
    dev = Dev(api, 2, (8, 8, 40), be_caps, stream)
    walks = [mr.Archive(), mr.Archive()]
    dev.update(mr.AFTER_INSERT, d, zero)
    walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, host, [0, 0])
    dev.update(mr.AFTER_INSERT, d3, zero)
    assert list(walk_and_compare(pkg.chain, dev, walks, mr.AFTER_INSERT, host3, [0, 0])) == [mr.INVALID, mr.UPDATED]
    # call level: nothing is enqueued, the status array keeps its bytes
    dev.status.fill_(STATUS_FILL)
    for kw, code in ((dict(batch=3), api.ERR_CAPACITY),):
        with pytest.raises(api.MyslamError) as e:
            dev.update(mr.AFTER_INSERT, d, zero, **kw)
        assert e.value.code == code
    other = Dev(api, 2, (8, 8, 40), (4, 41, 200), stream)                   # a back end whose mp_cap is not the archive's
    other.be_caps = (4, 40, 200)
    with pytest.raises(api.MyslamError) as e:
        other.update(mr.AFTER_INSERT, d, zero)
    assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.MyslamError):
        dev.update(7, d, zero)
    with pytest.raises(api.MyslamError):
        dev.update(mr.AFTER_OPTIMIZE, d, zero, report=None)
    stream.synchronize()
    assert (dev.status.cpu().numpy() == STATUS_FILL).all() and dev.h.launches_per_update() == 1


def test_slot_independence_and_load_get(api, pkg):
    import torch
    be_caps = (4, 40, 200)
    ms = [mi.small_map([3, 5, 8, 9], [mi.shifted(1.0 + i) for i in range(4)], 10, seed=s) for s in (1, 2, 3)]
    stream = torch.cuda.Stream(); stream.wait_stream(torch.cuda.current_stream())
    host3, d3 = hand_tables(ms, be_caps)
    host1, d1 = hand_tables([ms[2]], be_caps)
    dev3 = Dev(api, 3, (8, 8, 40), be_caps, stream); dev1 = Dev(api, 1, (8, 8, 40), be_caps, stream)
    dev3.update(mr.AFTER_INSERT, d3, torch.zeros(3, dtype=torch.int32, device="cuda"))
    dev1.update(mr.AFTER_INSERT, d1, torch.zeros(1, dtype=torch.int32, device="cuda"))
    (g3, _), (g1, _) = dev3.read(), dev1.read()
    assert mr.same(g3[2], g1[0]) is None and mr.same(g3[0], g1[0]) is not None
    # load -> get, and what load refuses
    a = g3[1]
    order = ("kf_id", "kf_pose", "edge_v0", "edge_v1", "meas", "mp_id", "mp_pos", "mp_first_kf", "mp_state", "snapshot", "mp_gone_kf", "mp_win_mask", "win_kf")
    dev1.h.load(0, *[a[k] for k in order])
    assert mr.same(dev1.h.get(0), a) is None
    for k, v in (("kf_id", a["kf_id"][::-1]), ("mp_id", np.r_[a["mp_id"][1:], a["mp_id"][:1]]), ("mp_state", np.full(10, 3, np.uint8)),
                 ("edge_v1", np.full(3, 9, np.int32)), ("mp_first_kf", np.full(10, 4, np.int32)), ("snapshot", np.full(10, 10, np.int32))):
        bad = dict(a); bad[k] = v
        with pytest.raises(api.MyslamError) as e:
            dev1.h.load(0, *[bad[j] for j in order])
        assert e.value.code == api.ERR_INVALID, k
    assert mr.same(dev1.h.get(0), a) is None                                # a refused load keeps every byte
    v = dev1.h.view()
    assert (v.kf_cap, v.edge_cap, v.point_cap, v.backend_mp_cap, v.max_batch) == (8, 8, 40, 40, 1) and v.kf_pose and v.mp_state


def test_recorded_step_replayed_twice(api, pkg, synth):
    """insert + update + optimise + update recorded once; two replays on restored tables give what two eager passes give"""
    import torch
    made = [br.make_map(synth, s, n_kf=4, n_mp=60) for s in (0x320, 0x321)]
    maps, K = [x[0] for x in made], made[0][1]
    rng = np.random.default_rng(7)
    inss = [next_keyframe(pkg.chain, m, K, 2, rng) for m in maps]
    be_caps, B = (8, 160, 1600), 2
    r = Run(api, maps, inss, 4, 0.2, caps=(be_caps, 64, 2, 4))
    full = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    oo = [full((B, be_caps[2]), torch.uint8), full((B, be_caps[1]), torch.uint8), full((B, be_caps[1]), torch.int32), full((B,), torch.int32),
          full((B, be_caps[2]), torch.float64), full((B,), torch.int32), full((B,), torch.int32), full((B,), torch.int32)]
    eager, rec = Dev(api, B, (16, 15, 300), be_caps, r.stream), Dev(api, B, (16, 15, 300), be_caps, r.stream)
    st2 = [torch.full((B,), STATUS_FILL, dtype=torch.int32, device="cuda") for _ in range(2)]

    def step(dev):
        r.enqueue()
        dev.update(mr.AFTER_INSERT, r.d, r.o["status"], r.di["outlier_mp_id"], r.di["n_outlier"], 4)
        st2[0].copy_(dev.status)
        r.h.optimize_batch(*[r.d[k].data_ptr() for k in TABLE_ARGS], B, K, *[t.data_ptr() for t in oo])
        dev.update(mr.AFTER_OPTIMIZE, r.d, oo[7], report=oo[1])
        st2[1].copy_(dev.status)

    r.stream.wait_stream(torch.cuda.current_stream())
    want = []
    for _ in range(2):
        r.restore()
        with torch.cuda.stream(r.stream):
            step(eager)
        want.append((eager.read()[0], st2[0].cpu().numpy().copy(), st2[1].cpu().numpy().copy()))
    # the second pass inserts the same key-frame into the restored tables: everything is found, nothing appended
    assert all((x == 0).all() for w in want for x in w[1:])
    r.restore()
    r.stream.synchronize()
    with torch.cuda.stream(r.stream):
        g = api.StepGraph.record(r.stream.cuda_stream, [], lambda: step(rec))
    assert g.node_count() >= 6
    for n in range(2):
        r.restore()
        g.launch(r.stream.cuda_stream)
        got = rec.read()[0]
        for b in range(B):
            assert mr.same(got[b], want[n][0][b]) is None, (n, b)
        assert (st2[0].cpu().numpy() == want[n][1]).all() and (st2[1].cpu().numpy() == want[n][2]).all()
