"""myslam_mapper_keyframe_batch (csrc/mapper.hip) against the entry points it composes.  The yardstick of every item is a SEPARATE single-item handle set
(api.Backend + api.MapArchive + api.ObsArchive, batch 1) driven through the existing calls — prior_rows, insert, map update, obs update, optimise, map
update, obs update — and only on the calls in which the item takes a key-frame.  After every mapper call the item's 13 tables (whole, beyond the counts
too), MapArchive.get (internals included) and ObsArchive.get must be the yardstick's byte for byte and the status words its statuses.
Mixed histories (tests/whole_map_model.py under the idle pattern of tests/mapper_ref.py), the hazard of an empty table and of a window an optimise would
move, the gate's table on the device, a capacity fault with its stickiness and reset_item, and a recorded call."""
import ctypes as C

import numpy as np
import pytest

import map_insert_ref as mi
import mapper_ref as mp
import test_mapper_ref as tm
import test_whole_map_model as T
import whole_map_model as wm
from test_gpu_map_histories import BE_CAPS, FEAT_CAP, LOAD, PRIOR_CAP, caps_for

pytestmark = pytest.mark.gpu

OUTLIER_CAP = 2 * FEAT_CAP          # the turn's layout: outlier stride = 2 x feature stride (the lists hold up to 64 ids)
ROW_CAP = 2048
TABLES = dict(kf_id=("k", (), np.int64), kf_pose=("k", (7,), np.float64), n_kf=(None, (), np.int32), mp_id=("m", (), np.int64), mp_pos=("m", (3,), np.float64),
              mp_outlier=("m", (), np.uint8), n_mp=(None, (), np.int32), obs_mp=("o", (), np.int32), obs_kf=("o", (), np.int32), obs_flags=("o", (), np.uint8),
              obs_uv=("o", (2,), np.float32), obs_tag=("o", (), np.int32), n_obs=(None, (), np.int32))
TURN = dict(new_kf_id="new_kf_id", new_kf_pose="new_kf_pose", feat_mp_id="feat_mp_id", feat_mp_pos="feat_mp_pos", feat_uv="feat_uv", feat_tag="feat_tag",
            feat_flags="feat_flags", n_feat="n_feat", outlier_mp_id="outlier_mp_id", n_outlier_mp="n_outlier")      # turn output -> mi.pack_inputs' name
# two banks of six: the three histories of one window twice, in other slots and under other idle draws (the window is an argument of the call, so
# a bank shares it, as a bank of streams shares Map.activeMap.size)
BANKS = (tuple(T.HISTORIES[:3]) * 2, tuple(T.HISTORIES[3:6]) * 2)


def _torch_dtype(torch, dt):
    return {np.int64: torch.int64, np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}[dt]


def peek(api, ptr, shape, dtype):
    out = np.zeros(shape, dtype)
    api._check(api.lib().myslam_debug_peek(C.c_void_p(ptr), out.ctypes.data_as(C.c_void_p), out.nbytes), "myslam_debug_peek")
    return out


class Rig:
    """a mapper of S items with its turn buffers, and one single-item yardstick per item, all on one stream"""

    def __init__(self, api, S, be_caps, feat_cap, arch_caps, row_cap, prior_cap, window, yards=True):
        import torch
        self.torch, self.api, self.S, self.caps, self.F, self.P, self.X, self.window = torch, api, S, be_caps, feat_cap, prior_cap, 2 * feat_cap, window
        self.arch_caps, self.row_cap = arch_caps, row_cap
        self.stream = torch.cuda.Stream()
        self.m = api.Mapper(S, *be_caps, feat_cap, *arch_caps, row_cap, prior_cap, stream=self.stream.cuda_stream)
        self.v = self.m.view()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        F, X = feat_cap, self.X
        self.turn = dict(new_kf_id=z(S, torch.int64), new_kf_pose=z((S, 7), torch.float64), feat_mp_id=z((S, F), torch.int64), feat_mp_pos=z((S, F, 3), torch.float64),
                         feat_uv=z((S, F, 2), torch.float32), feat_tag=z((S, F), torch.int32), feat_flags=z((S, F), torch.uint8), n_feat=z(S, torch.int32),
                         outlier_mp_id=z((S, X), torch.int64), n_outlier_mp=z(S, torch.int32), report=z((S, 8), torch.int32))
        self.d_status = torch.full((S, api.MAPPER_STATUS_WORDS), -77, dtype=torch.int32, device="cuda")
        self.yards = [Yard(self) for _ in range(S)] if yards else []
        self.stream.wait_stream(torch.cuda.current_stream())

    def shape(self, name):
        dim, tail, dt = TABLES[name]
        n = {"k": self.caps[0], "m": self.caps[1], "o": self.caps[2], None: None}[dim]
        return ((self.S,) if n is None else (self.S, n)) + tail, dt

    def tables(self):
        """the mapper's 13 tables, whole (synchronises)"""
        self.stream.synchronize()
        return {k: peek(self.api, getattr(self.v, k), *self.shape(k)) for k in TABLES}

    def fill(self, items):
        """items: per item (turn status, map_insert_ref.Insert or None) -> the turn buffers"""
        torch = self.torch
        inss = [mi.Insert(i.kf_id, i.kf_pose, i.feats, [], i.outlier_ids) if i is not None else mi.Insert(-1, mi.IDENT, []) for _, i in items]
        host = mi.pack_inputs(inss, self.F, self.P, self.X)
        rep = np.zeros((self.S, 8), np.int32); rep[:, 0] = [s for s, _ in items]
        with torch.cuda.stream(self.stream):
            for k, src in TURN.items():
                self.turn[k].copy_(torch.from_numpy(host[src]))
            self.turn["report"].copy_(torch.from_numpy(rep))

    def outs(self):
        return {k: v.data_ptr() for k, v in self.turn.items()}

    def call(self):
        self.m.keyframe_batch(None, self.outs(), self.window, T.K, self.d_status.data_ptr())

    def words(self):
        self.stream.synchronize()
        return self.d_status.cpu().numpy().copy()

    def same_as_yard(self, b, tabs, where):
        y = self.yards[b]
        for k in TABLES:
            assert tabs[k][b].tobytes() == y.d[k].cpu().numpy()[0].tobytes(), (where, b, k)
        for got, want, what in ((self.m.map.get(b), y.map.get(0), "map"), (self.m.obs.get(b), y.obs.get(0), "obs")):
            for k in want:
                x, w = np.asarray(got[k]), np.asarray(want[k])
                assert x.dtype == w.dtype and x.shape == w.shape and x.tobytes() == w.tobytes(), (where, b, what, k)


class Yard:
    """one item through the existing entry points"""

    def __init__(self, rig):
        torch, api, st = rig.torch, rig.api, rig.stream.cuda_stream
        self.rig = rig
        K, M, N = rig.caps
        self.be = api.Backend(1, K, M, N, stream=st)
        self.map = api.MapArchive(1, *rig.arch_caps, M, stream=st)
        self.obs = api.ObsArchive(self.map, 1, N, rig.row_cap, stream=st)
        self.map.attach_solve(*self.be.solve_view())
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.d = {k: z((1,) + rig.shape(k)[0][1:], _torch_dtype(torch, rig.shape(k)[1])) for k in TABLES}
        P, F = rig.P, rig.F
        self.prior = [z((1, P), torch.int64), z((1, P), torch.int64), z((1, P, 2), torch.float32), z((1, P), torch.int32), z((1, P), torch.uint8), z(1, torch.int32)]
        self.ins_out = [z((1, F), torch.int32), z((1, M), torch.int32), z(1, torch.int64), z(1, torch.int32), z((1, K), torch.float64)]
        self.opt_out = [z((1, N), torch.uint8), z((1, M), torch.uint8), z((1, M), torch.int32), z(1, torch.int32), z((1, N), torch.float64), z(1, torch.int32),
                        z(1, torch.int32)]
        self.st = torch.full((7,), -88, dtype=torch.int32, device="cuda")

    def take(self, b):
        """item b of the rig's turn buffers is this item's new key-frame: the seven existing calls, in the header's order"""
        rig, api = self.rig, self.rig.api
        K, M, N = rig.caps
        t = {k: v[b].data_ptr() for k, v in rig.turn.items()}
        d = {k: v.data_ptr() for k, v in self.d.items()}
        tabs = [d[k] for k in TABLES]
        s = [self.st[i:i + 1].data_ptr() for i in range(7)]
        pr = [x.data_ptr() for x in self.prior]
        self.obs.prior_rows_batch(t["feat_mp_id"], t["n_feat"], rig.F, d["mp_id"], d["n_mp"], M, 1, *pr, rig.P, s[0])
        self.be.insert_keyframe_batch(*tabs, t["new_kf_id"], t["new_kf_pose"], t["feat_mp_id"], t["feat_mp_pos"], t["feat_uv"], t["feat_tag"], t["feat_flags"],
                                      t["n_feat"], rig.F, *pr, rig.P, t["outlier_mp_id"], t["n_outlier_mp"], rig.X, 1, rig.window, 0.2,
                                      *[x.data_ptr() for x in self.ins_out], s[1])
        mt = [d["kf_id"], d["kf_pose"], d["n_kf"], K, d["mp_id"], d["mp_pos"], d["n_mp"], M, d["obs_mp"], d["obs_kf"], d["obs_flags"], d["n_obs"], N]
        self.map.update_batch(api.MAP_AFTER_INSERT, *mt, s[1], t["outlier_mp_id"], t["n_outlier_mp"], rig.X, None, 1, s[2])
        self.obs.update_batch(api.MAP_AFTER_INSERT, *tabs, K, M, N, s[1], s[2], None, 1, s[3])
        oo = [x.data_ptr() for x in self.opt_out]
        self.be.optimize_batch(*tabs, 1, T.K, *oo, s[4])
        self.map.update_batch(api.MAP_AFTER_OPTIMIZE, *mt, s[4], None, None, 0, oo[1], 1, s[5])
        self.obs.update_batch(api.MAP_AFTER_OPTIMIZE, *tabs, K, M, N, s[4], s[5], oo[0], 1, s[6])

    def statuses(self):
        return self.st.cpu().numpy().tolist()


def correct_on_device(rig, map_handle, item, tables, batch, corr):
    """a correction from outside (the loop closer's): the archive item takes the moved values, write_backend carries them to the tables, rows found by id"""
    torch = rig.torch
    rig.stream.synchronize()
    for c in corr:
        arch = map_handle.get(item)
        for row, kid in enumerate(arch["kf_id"]):
            arch["kf_pose"][row] = c.kf_pose[int(kid)]
        for s, mid in enumerate(arch["mp_id"]):
            if int(mid) in c.mp_pos:
                arch["mp_pos"][s] = c.mp_pos[int(mid)]
        map_handle.load(item, *[arch[k] for k in LOAD])
        sel = np.zeros(batch, np.uint8); sel[item] = 1
        d_sel = torch.from_numpy(sel).cuda()
        rig.stream.wait_stream(torch.cuda.current_stream())
        map_handle.write_backend_batch(tables["kf_id"], tables["kf_pose"], tables["n_kf"], rig.caps[0], tables["mp_id"], tables["mp_pos"], tables["n_mp"], rig.caps[1],
                                       d_sel.data_ptr(), batch)
        rig.stream.synchronize()


def first_negative(st):
    return next((v for v in st if v < 0), 0)


@pytest.mark.parametrize("n", range(len(BANKS)))
def test_mixed_histories_equal_the_existing_calls(api, pkg, oracle, n):
    specs = BANKS[n]
    window = specs[0][1]
    assert all(s[1] == window for s in specs)
    arch_caps = caps_for(pkg, oracle, list(dict.fromkeys(specs)))
    rig = Rig(api, 6, BE_CAPS, FEAT_CAP, arch_caps, ROW_CAP, PRIOR_CAP, window)
    torch = rig.torch
    scripts = [tm.script(pkg, oracle, s) for s in specs]
    at, idles, last_ins, fault = [0] * 6, [0] * 6, [None] * 6, [0] * 6
    seen = dict(calls=0, all_idle=0, all_take=0, mixed=0, takes=0, capacity=0, refused=0, empty=0, moved_by_optimise=0, stale_idle=0)
    mt = {k: getattr(rig.v, k) for k in TABLES}
    scratch = api.Backend(1, *BE_CAPS, stream=rig.stream.cuda_stream)
    for take in mp.rounds(6, [len(s) for s in scripts], tm.PATTERN_SEED + n):
        items, kinds = [], []
        for b in range(6):
            if take[b]:
                corr, e, _ = scripts[b][at[b]]
                at[b] += 1
                if corr and not fault[b]:
                    correct_on_device(rig, rig.m.map, b, mt, 6, corr)
                    y = rig.yards[b]
                    correct_on_device(rig, y.map, 0, {k: v.data_ptr() for k, v in y.d.items()}, 1, corr)
                if e.kind == "refused":
                    items.append((mp.NO_TURN, e.ins)); kinds.append("idle"); seen["refused"] += 1
                else:
                    items.append((0, e.ins)); kinds.append("idle" if fault[b] else e.kind)
                    last_ins[b] = e.ins
            else:
                status, ins = mp.idle_buffers(idles[b], last_ins[b])
                idles[b] += 1; seen["stale_idle"] += ins is not None
                items.append((status, ins)); kinds.append("idle")
        rig.fill(items)
        if all(k == "idle" for k in kinds) and seen["calls"] >= 2:
            # THE HAZARD: what the existing optimise call would do to these idle items — it moves the window of every one that holds edges
            for b in range(6):
                y = rig.yards[b]
                if not fault[b] and all(at[i] == len(scripts[i]) for i in range(6)):     # the closing calls: five active points pushed 5 cm from
                    # outside, on both sides, so that the window is surely not converged (in between the histories stay the model's)
                    arch = rig.m.map.get(b)
                    rig.stream.synchronize()
                    ids = y.d["mp_id"].cpu().numpy()[0, :int(y.d["n_mp"].item())][:5]
                    at_id = {int(i): s for s, i in enumerate(arch["mp_id"])}
                    push = mp.Entry("correct", kf_pose={int(k): arch["kf_pose"][r] for r, k in enumerate(arch["kf_id"])},
                                    mp_pos={int(i): arch["mp_pos"][at_id[int(i)]] + 0.05 for i in ids})
                    correct_on_device(rig, rig.m.map, b, mt, 6, [push])
                    correct_on_device(rig, y.map, 0, {k: v.data_ptr() for k, v in y.d.items()}, 1, [push])
                with torch.cuda.stream(rig.stream):
                    cp = {k: v.clone() for k, v in y.d.items()}
                    o = [torch.zeros_like(x) for x in y.opt_out] + [torch.zeros(1, dtype=torch.int32, device="cuda")]
                scratch.optimize_batch(*[cp[k].data_ptr() for k in TABLES], 1, T.K, *[x.data_ptr() for x in o])
                rig.stream.synchronize()
                seen["moved_by_optimise"] += int(o[-1].item() == 0 and cp["kf_pose"].cpu().numpy().tobytes() != y.d["kf_pose"].cpu().numpy().tobytes())
        rig.call()
        for b in range(6):
            if kinds[b] != "idle":
                rig.yards[b].take(b)
        words, tabs = rig.words(), rig.tables()
        for b in range(6):
            where = (specs[b][0], "call %d" % seen["calls"], kinds[b])
            if kinds[b] == "idle":
                assert words[b].tolist() == [fault[b] if fault[b] else api.MAPPER_IDLE] + [api.MAPPER_IDLE] * 7, (where, words[b])
            else:
                st = rig.yards[b].statuses()
                assert words[b].tolist() == [first_negative(st)] + st, (where, words[b], st)
                if kinds[b] == "capacity":
                    assert words[b, 0] == words[b, 3] == mp.ERR_CAPACITY and words[b, 2] == 0, (where, words[b])
                    fault[b] = mp.ERR_CAPACITY; seen["capacity"] += 1
                else:
                    assert words[b, 0] == 0 and st[4] == scripts[b][at[b] - 1][1].opt_status, (where, st)
                    seen["takes"] += 1; seen["empty"] += st[4] == 1
            rig.same_as_yard(b, tabs, where)                                # idle or not: the yardstick was only called when the item took a key-frame
        seen["calls"] += 1
        seen["all_idle"] += all(k == "idle" for k in kinds); seen["all_take"] += all(k != "idle" for k in kinds); seen["mixed"] += len(set(k == "idle" for k in kinds)) == 2
    print("bank %d:" % n, seen, "idle calls per item", idles, "archive caps", arch_caps)
    for b, spec in enumerate(specs):
        assert at[b] == len(scripts[b]) and len(rig.m.get(b)["kf_id"]) == spec[2] and idles[b] >= 2, (spec, at[b])
    assert seen["all_idle"] >= 3 and seen["all_take"] >= 1 and seen["mixed"] >= 8 and seen["stale_idle"] >= 6
    assert seen["capacity"] == sum("capacity" in s[4] for s in specs) and seen["empty"] >= sum("empty" in s[4] for s in specs)
    assert seen["moved_by_optimise"] >= 3                                   # the windows the idle calls kept are windows the existing call moves


def small_keyframe(chain, kf_id, x, ids, new_pos=None, tag0=0):
    """a key-frame at a pure translation x that sees the points `ids` (id -> position) where they project"""
    pose = mi.shifted(x)
    feats = []
    for j, (mid, pw) in enumerate(sorted(ids.items())):
        uv, _ = wm.project(chain, T.K, pose, np.asarray(pw, float))
        feats.append((int(mid), tuple(float(v) for v in pw), (np.float32(uv[0]), np.float32(uv[1])), tag0 + j, False))
    return mi.Insert(kf_id, pose, feats)


def grid_points(first_id, n):
    return {first_id + i: (-3.0 + 0.37 * i, -1.0 + 0.21 * (i % 5), 9.0 + 0.6 * (i % 4)) for i in range(n)}


def test_an_empty_table_stays_empty_for_items_without_a_key_frame(api, pkg):
    """the (-1, pose) row the insert would append to an EMPTY table (include/myslam_hip.h, tracker section) never gets there"""
    rig = Rig(api, 3, (4, 32, 96), 24, (8, 8, 64), 128, 16, 3, yards=False)
    kf = small_keyframe(pkg.chain, 0, 0.0, grid_points(100, 12))
    rig.fill([(mp.NO_TURN, None), (mp.INIT_RETRY, None), (0, kf)])
    rig.call()
    words, tabs = rig.words(), rig.tables()
    assert words[0].tolist() == words[1].tolist() == [api.MAPPER_IDLE] * 8 and words[2, 0] == 0, words
    for b in (0, 1):
        assert tabs["n_kf"][b] == 0 and all(not tabs[k][b].any() for k in TABLES), b
        assert len(rig.m.get(b)["kf_id"]) == 0 and rig.m.obs.get(b)["rows_in_use"] == 0
    assert tabs["n_kf"][2] == 1 and tabs["n_mp"][2] == 12 and tabs["n_obs"][2] == 12 and rig.m.get(2)["kf_id"].tolist() == [0]


def test_the_gate_table_on_the_device(api, pkg):
    """16 rows in two calls of 8 items: items 0-3 healthy, items 4-7 faulted first (a key-frame whose id is not above the table's last)"""
    rig = Rig(api, 8, (4, 32, 96), 24, (8, 8, 64), 128, 16, 3, yards=False)
    chain, pts = pkg.chain, grid_points(100, 6)
    rig.fill([(0, small_keyframe(chain, 5, 0.0, pts))] * 8)
    rig.call()
    assert (rig.words()[:, 0] == 0).all()
    rig.fill([(mp.NO_TURN, None)] * 4 + [(0, small_keyframe(chain, 5, 0.5, pts))] * 4)
    rig.call()
    w = rig.words()
    assert (w[:4, 0] == api.MAPPER_IDLE).all() and (w[4:, 0] == mp.ERR_INVALID).all() and (w[4:, 2] == mp.ERR_INVALID).all() and (w[4:, 5] == api.MAPPER_IDLE).all(), w
    statuses = (0, mp.NO_TURN, mp.INIT_RETRY, mp.ERR_CAPACITY)
    before = rig.tables()
    rows = {}
    for has_id in (False, True):                                            # id -1 first: the tables of the healthy items are still comparable
        kf = small_keyframe(chain, 9, 1.0, pts) if has_id else mi.Insert(-1, mi.IDENT, small_keyframe(chain, 9, 1.0, pts).feats)
        rig.fill([(s, kf) for s in statuses] * 2)
        rig.call()
        gate = peek(api, rig.v.gate, (8,), np.int32)
        w, after = rig.words(), rig.tables()
        for b in range(8):
            rows[(statuses[b % 4], has_id, b >= 4)] = int(gate[b])
            if gate[b]:
                assert w[b].tolist() == [mp.ERR_INVALID if b >= 4 else api.MAPPER_IDLE] + [api.MAPPER_IDLE] * 7, (b, w[b])
                assert all(after[k][b].tobytes() == before[k][b].tobytes() for k in TABLES), b
            else:
                assert w[b, 0] == 0 and after["n_kf"][b] == 2, (b, w[b])
    assert len(rows) == 16
    for status, kf_id, fault, want in mp.GATE_TABLE:
        assert rows[(status, kf_id >= 0, fault != 0)] == want == mp.gate(status, kf_id, fault), (status, kf_id, fault)


def test_a_capacity_fault_sticks_until_reset_and_neighbours_are_served(api, pkg):
    """obs_cap 40: item 0's second key-frame brings the rows to 41, item 1's to exactly 40, item 2 is far from the cap"""
    rig = Rig(api, 3, (4, 48, 40), 24, (8, 8, 64), 128, 16, 3)
    chain = pkg.chain
    old, extra = grid_points(100, 20), {200: (0.5, 0.25, 11.0)}
    first = small_keyframe(chain, 0, 0.0, old)
    rig.fill([(0, first)] * 3)
    rig.call()
    for b in range(3):
        rig.yards[b].take(b)
    assert (rig.words()[:, 0] == 0).all()
    rig.fill([(0, small_keyframe(chain, 1, 0.5, {**old, **extra}, tag0=100)), (0, small_keyframe(chain, 1, 0.5, old, tag0=100)),
              (0, small_keyframe(chain, 1, 0.5, dict(list(old.items())[:5]), tag0=100))])
    before = rig.tables()
    kept = (rig.m.map.get(0), rig.m.obs.get(0))
    rig.call()
    for b in (1, 2):
        rig.yards[b].take(b)
    w, tabs = rig.words(), rig.tables()
    assert w[0].tolist() == [mp.ERR_CAPACITY, 0, mp.ERR_CAPACITY, api.MAP_SKIPPED, api.MAP_SKIPPED, api.MAPPER_IDLE, api.MAP_SKIPPED, api.MAP_SKIPPED], w[0]
    assert w[1, 0] == 0 and tabs["n_obs"][1] == 40 and w[2, 0] == 0, w

    def item0_kept():
        t = rig.tables()
        assert all(t[k][0].tobytes() == before[k][0].tobytes() for k in TABLES)
        for got, want in zip((rig.m.map.get(0), rig.m.obs.get(0)), kept):
            assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want)
        return t

    tabs = item0_kept()
    for b in (1, 2):
        rig.same_as_yard(b, tabs, "the faulting call")
    for r in (2, 3):                                                        # two later calls: the fault is reported, the bytes stay, the neighbours go on
        none = small_keyframe(chain, r, 0.5 * r, {})
        rig.fill([(0, small_keyframe(chain, r, 0.5 * r, dict(list(old.items())[:3]), tag0=200 * r)), (0, none) if r == 2 else (mp.NO_TURN, None),
                  (0, small_keyframe(chain, r, 0.5 * r, dict(list(old.items())[:5]), tag0=200 * r))])
        rig.call()
        if r == 2:
            rig.yards[1].take(1)
        rig.yards[2].take(2)
        w = rig.words()
        assert w[0].tolist() == [mp.ERR_CAPACITY] + [api.MAPPER_IDLE] * 7 and w[2, 0] == 0 and w[1, 0] == (0 if r == 2 else api.MAPPER_IDLE), w
        tabs = item0_kept()
        for b in (1, 2):
            rig.same_as_yard(b, tabs, "call %d after the fault" % r)
    rig.m.reset_item(0)
    t = rig.tables()
    assert all(not t[k][0].any() for k in TABLES) and len(rig.m.get(0)["kf_id"]) == 0 and rig.m.obs.get(0)["error"] == 0
    assert peek(api, rig.v.fault, (3,), np.int32).tolist() == [0, 0, 0]
    rig.yards[0] = Yard(rig)
    rig.stream.wait_stream(rig.torch.cuda.current_stream())
    rig.fill([(0, small_keyframe(chain, 7, 0.0, old)), (mp.NO_TURN, None), (mp.INIT_RETRY, None)])
    rig.call()
    rig.yards[0].take(0)
    w, tabs = rig.words(), rig.tables()
    assert w[0, 0] == 0 and tabs["n_kf"][0] == 1 and tabs["kf_id"][0, 0] == 7, w
    for b in range(3):
        rig.same_as_yard(b, tabs, "after reset_item")


def test_a_recorded_call_replays_like_the_eager_one(api, pkg, oracle):
    """one eager call, then the mapper call alone recorded once and replayed for three later rounds of the same histories with the inputs copied into the
    same buffers: every byte is an eager handle set's, and the graph has as many nodes as the call has launches"""
    specs = BANKS[1]
    arch_caps = caps_for(pkg, oracle, list(dict.fromkeys(specs)))
    rec = Rig(api, 6, BE_CAPS, FEAT_CAP, arch_caps, ROW_CAP, PRIOR_CAP, specs[0][1], yards=False)
    eag = Rig(api, 6, BE_CAPS, FEAT_CAP, arch_caps, ROW_CAP, PRIOR_CAP, specs[0][1], yards=False)
    torch = rec.torch
    scripts = [tm.script(pkg, oracle, s) for s in specs]
    takes = [[e for _, e, _ in sc if e.kind == "take"] for sc in scripts]   # (corrections are left out on both sides: the inputs only have to be equal)
    pattern = ([True] * 6, [True, False, True, True, False, True], [False, True, True, False, True, False], [True, True, False, True, True, True])
    at, graph = [0] * 6, None
    for r, take in enumerate(pattern):
        items = []
        for b in range(6):
            if take[b]:
                items.append((0, takes[b][at[b]].ins)); at[b] += 1
            else:
                items.append(mp.idle_buffers(r + b, takes[b][at[b] - 1].ins))
        rec.fill(items); eag.fill(items)
        eag.call()
        if r == 0:
            rec.call()
            rec.stream.synchronize()
            with torch.cuda.stream(rec.stream):
                graph = api.StepGraph.record(rec.stream.cuda_stream, [], rec.call)
            assert graph.node_count() == rec.m.launches_per_call(False) == 11 and rec.m.launches_per_call(True) == 13
        else:
            graph.launch(rec.stream.cuda_stream)
        wr, we, tr, te = rec.words(), eag.words(), rec.tables(), eag.tables()
        assert wr.tobytes() == we.tobytes() and [int(v) for v in we[:, 0]] == [0 if t else api.MAPPER_IDLE for t in take], (r, we)
        for k in TABLES:
            assert tr[k].tobytes() == te[k].tobytes(), (r, k)
        for b in range(6):
            for got, want in ((rec.m.map.get(b), eag.m.map.get(b)), (rec.m.obs.get(b), eag.m.obs.get(b))):
                assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want), (r, b)
    assert min(at) >= 2


def test_call_level_refusals(api):
    import torch
    rig = Rig(api, 2, (4, 32, 96), 24, (8, 8, 64), 128, 16, 3, yards=False)
    outs = rig.outs()
    for bad in (dict(window=0), dict(rounds=0), dict(iters=0)):
        kw = dict(window=3, rounds=5, iters=10); kw.update(bad)
        with pytest.raises(api.MyslamError) as e:
            rig.m.keyframe_batch(None, outs, kw["window"], T.K, rig.d_status.data_ptr(), rounds=kw["rounds"], iters=kw["iters"])
        assert e.value.code == -1
    for k in ("new_kf_id", "n_feat", "report", "outlier_mp_id"):
        with pytest.raises(api.MyslamError) as e:
            rig.m.keyframe_batch(None, {**outs, k: 0}, 3, T.K, rig.d_status.data_ptr())
        assert e.value.code == -1
    with pytest.raises(api.MyslamError) as e:
        rig.m.keyframe_batch(None, outs, 3, T.K, 0)
    assert e.value.code == -1
    for caps, code in (((11, 32, 96), -4), ((4, 32, 16), -3)):              # the back end's window limit; feat_cap beyond obs_cap
        with pytest.raises(api.MyslamError) as e:
            api.Mapper(2, *caps, 24, 8, 8, 64, 128, 16)
        assert e.value.code == code
    rig.stream.synchronize()
    with torch.cuda.stream(rig.stream):
        codes = []

        def body():
            try:
                rig.m.reset_item(0)
            except api.MyslamError as err:
                codes.append(err.code)
            rig.call()                                                      # (the recording holds the call, not an empty graph)
        api.StepGraph.record(rig.stream.cuda_stream, [], body)
    assert codes == [-4]                                                    # reset_item while the stream is being recorded
