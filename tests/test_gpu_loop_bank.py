"""The loop key-frame store bank (csrc/loop_bank.hip, api.LoopStoreBank) on the device against tests/loop_bank_ref.py, byte for byte: every stage is
integer code and copies, so nothing here has a tolerance.  Every input array is random in every byte, slots beyond the counts included; every output
buffer is pre-filled with a pattern and compared WHOLE; after every call the whole allocation (read_view: every slot of every stream, bytes behind the
counts included, counts, last_closed, the finish plan) is compared with a host mirror, and get() of every stream with the model."""
import os
import subprocess

import numpy as np
import pytest

import lcd_bank_ref as LB
import lcddb_scan_ref as R
import loop_bank_ref as B
import loop_store_ref as LS

pytestmark = pytest.mark.gpu
THR = np.float32(0.94)
SENT = int(np.frombuffer(b"\xa5" * 4, np.int32)[0])
KEYS = ("desc", "n_loop", "pyr", "lm", "slot", "status")
DIM = R.DIM


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == LS.KP_DTYPE:
        a = a.view(np.uint8).reshape(a.shape + (28,))
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def _sent(n):
    import torch
    return torch.full((n,), SENT, dtype=torch.int32, device="cuda")


def _code(api, fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0
    except api.MyslamError as e:
        return e.code


def _clamp(v, hi):
    return min(max(int(v), 0), hi)


class Pair:
    """the device bank and the model, fed the same calls; `m` = what the whole allocation must hold"""

    def __init__(self, api, S, K, cap, F, stream=None, every_get=True):
        import torch
        self.api, self.torch, self.S, self.K, self.cap, self.F, self.every_get = api, torch, S, K, cap, F, every_get
        self.dev = api.LoopStoreBank(S, K, cap, F, stream)
        self.ref = B.Bank(S, K, cap, F)
        v = self.dev.view()
        assert (v.streams, v.kfs_per_stream, v.cap, v.feat_cap) == (S, K, cap, F) and v.cap_stride == (cap + 3) // 4 * 4 and v.feat_stride == (F + 3) // 4 * 4
        cs, fs = v.cap_stride, v.feat_stride
        self.m = dict(kps=np.zeros((S, K, cs), LS.KP_DTYPE), desc=np.zeros((S, K, cs, 32), np.uint8), lm=np.zeros((S, K, fs), np.int32),
                      rows=np.zeros((S, K), np.int32), nfeat=np.zeros((S, K), np.int32), ids=np.zeros((S, K), np.uint64))
        self.keep = []

    def sync(self):
        self.torch.cuda.synchronize()

    # ---- state ----
    def load(self, s, ids, kps, desc, rows, lm, nf, last_closed=-1):
        self.dev.load(s, ids, kps, desc, rows, lm, nf, last_closed)
        self.ref.load(s, ids, kps, desc, rows, lm, nf, last_closed)
        n = len(ids)
        if n:
            self.m["kps"][s, :n, :self.cap] = kps; self.m["desc"][s, :n, :self.cap] = desc; self.m["lm"][s, :n, :self.F] = lm
            self.m["rows"][s, :n] = rows; self.m["nfeat"][s, :n] = nf; self.m["ids"][s, :n] = ids

    def check(self, what="", gets=None):
        self.sync()
        got = self.dev.read_view()
        for k, want in self.m.items():
            assert got[k].tobytes() == want.tobytes(), (what, k)
        assert got["n"].tolist() == self.ref.sizes() == self.dev.sizes().tolist(), (what, got["n"], self.ref.sizes())
        assert got["last_closed"].tolist() == self.ref.last_closed, (what, got["last_closed"], self.ref.last_closed)
        assert got["put_slot"].tolist() == self.ref.put_slot, (what, got["put_slot"], self.ref.put_slot)
        if self.every_get if gets is None else gets:
            for s in range(self.S):
                g, kfs = self.dev.get(s), self.ref.stores[s].kfs
                assert g["ids"].tolist() == list(kfs) and g["last_closed"] == self.ref.last_closed[s], (what, s)
                for r, kf in enumerate(kfs.values()):
                    n, nf = len(kf["kps"]), len(kf["lm"])
                    assert (g["rows"][r], g["nfeat"][r]) == (n, nf), (what, s, r)
                    assert g["kps"][r, :n].tobytes() == kf["kps"].tobytes() and g["desc"][r, :n].tobytes() == kf["desc"].tobytes(), (what, s, r)
                    assert g["lm"][r, :nf].tolist() == kf["lm"].tolist(), (what, s, r)

    # ---- the calls ----
    def gate(self, new_id, item_status=None, stride=1, what=""):
        d_id = _dev(np.asarray(new_id, np.int64))
        d_st = None if item_status is None else _dev(np.asarray(item_status, np.int32))
        act, st = _sent(self.S), _sent(self.S)
        self.dev.gate_batch(d_id.data_ptr(), 0 if d_st is None else d_st.data_ptr(), stride, act.data_ptr(), st.data_ptr())
        self.sync()
        want = self.ref.gate(new_id, item_status, stride)
        assert (act.cpu().tolist(), st.cpu().tolist()) == want, (what, act.cpu().tolist(), st.cpu().tolist(), want)
        return want[0], want[1], act

    def outputs(self):
        return {k: _dev(v) for k, v in LS.sentinel_outputs(self.S, self.cap, self.F).items()}

    def launch_detect(self, q, out, thr_high=THR, max_suspected=3, desc_ptr=None):
        self.dev.detect_batch(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), desc_ptr or out["desc"].data_ptr(),
                              out["n_loop"].data_ptr(), out["pyr"].data_ptr(), out["lm"].data_ptr(), out["slot"].data_ptr(), out["status"].data_ptr(),
                              thr_high, max_suspected)

    def detect(self, best_id, best_row, score, cnt, thr_high=THR, max_suspected=3, what=""):
        """one call on pattern-filled outputs, compared whole with the model -> the expected arrays"""
        best_id, best_row = np.asarray(best_id, np.uint64), np.asarray(best_row, np.int32)
        score, cnt = np.asarray(score, np.float32), np.asarray(cnt, np.int32)
        q = [_dev(best_id), _dev(best_row), _dev(score), _dev(cnt)]
        out = self.outputs()
        self.launch_detect(q, out, thr_high, max_suspected)
        self.sync()
        want = self.ref.detect(best_id, best_row, score, cnt, thr_high, max_suspected, LS.sentinel_outputs(self.S, self.cap, self.F))
        for k in KEYS:
            assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), (what, k)
        return want

    def note_finish(self, n0, status, cur_id, kps, desc, counts, kf_status, lm, nf):
        for s in range(self.S):
            if status[s] == B.STORED:
                r = n0[s]
                n = 0 if kf_status is not None and kf_status[s] != 0 else _clamp(counts[s], self.cap)
                f = _clamp(nf[s], self.F)
                self.m["kps"][s, r, :n] = kps[s, :n]; self.m["desc"][s, r, :n] = desc[s, :n]; self.m["lm"][s, r, :f] = lm[s, :f]
                self.m["rows"][s, r] = n; self.m["nfeat"][s, r] = f; self.m["ids"][s, r] = cur_id[s]

    def finish(self, cur_id, active, verify, kps, desc, counts, kf_status, lm, nf, what="", desc_off=0):
        """-> (add, status) of the model, equal to the device's, and the device's d_add"""
        cur_id = np.asarray(cur_id).astype(np.uint64)
        raw = np.zeros(desc.size + 16, np.uint8); raw[desc_off:desc_off + desc.size] = desc.reshape(-1)
        t = [_dev(cur_id), _dev(np.asarray(active, np.int32)), _dev(np.asarray(verify, np.int32)), _dev(kps), _dev(raw), _dev(np.asarray(counts, np.int32)),
             None if kf_status is None else _dev(np.asarray(kf_status, np.int32)), _dev(lm), _dev(np.asarray(nf, np.int32))]
        self.keep = [t]
        add, st = _sent(self.S), _sent(self.S)
        self.dev.finish_batch(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr() + desc_off, t[5].data_ptr(),
                              0 if t[6] is None else t[6].data_ptr(), t[7].data_ptr(), t[8].data_ptr(), add.data_ptr(), st.data_ptr())
        self.sync()
        n0 = self.ref.sizes()
        want = self.ref.finish(cur_id, active, verify, kps, desc, counts, kf_status, lm, nf)
        self.note_finish(n0, want[1], cur_id, kps, desc, counts, kf_status, lm, nf)
        assert (add.cpu().tolist(), st.cpu().tolist()) == want, (what, add.cpu().tolist(), st.cpu().tolist(), want)
        return want[0], want[1], add

    def set_links(self, lists, values=True, n=None, list_cap=8, pending_ids=None, pending=None, what=""):
        """lists[s]: [(kf id, tag, value)]; values False: no value column (clear_links, every value must be -1) -> hits"""
        S = self.S
        ids = np.full((S, list_cap), -5, np.int64); tags = np.full((S, list_cap), -5, np.int32); vals = np.full((S, list_cap), -5, np.int32)
        for s, l in enumerate(lists):
            for j, (i, t, v) in enumerate(l[:list_cap]):
                ids[s, j], tags[s, j], vals[s, j] = i, t, v
        cnt = np.array([len(l) for l in lists], np.int32) if n is None else np.asarray(n, np.int32)
        d = [_dev(ids), _dev(tags), _dev(vals), _dev(cnt)]
        d_pid = None if pending_ids is None else _dev(np.asarray(pending_ids, np.int64))
        d_p = None if pending is None else _dev(pending)
        hits = _sent(S)
        self.dev.set_links_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if values else 0, d[3].data_ptr(), list_cap,
                                 0 if d_pid is None else d_pid.data_ptr(), 0 if d_p is None else d_p.data_ptr(), hits.data_ptr())
        self.sync()
        want = self.ref.set_links([l[:list_cap] for l in lists], cnt, list_cap, pending_ids, pending)
        assert hits.cpu().tolist() == want, (what, hits.cpu().tolist(), want)
        if pending is not None:
            assert d_p.cpu().numpy().tobytes() == pending.tobytes(), what
        for s in range(S):
            for r, kf in enumerate(self.ref.stores[s].kfs.values()):
                self.m["lm"][s, r, :len(kf["lm"])] = kf["lm"]
        return want

    def clear(self, flags):
        d = _dev(np.asarray(flags, np.int32))
        self.dev.clear_batch(d.data_ptr())
        self.sync()
        self.ref.clear(flags)


def _kfs(seed, S, cap, F):
    return LS.random_keyframes(seed, S, cap, F)


def _fill(p, per_stream, seed=50):
    """per_stream[s] = [(id, rows, nfeat)]: loaded whole, every byte of every slot random"""
    for s, l in enumerate(per_stream):
        kps, desc, lm = _kfs(seed + s, len(l), p.cap, p.F)
        p.load(s, [x[0] for x in l], kps, desc, [x[1] for x in l], lm, [x[2] for x in l])


# ---- 1. gate ---------------------------------------------------------------------------------------------------------------------------
def test_gate_edges_per_stream(api):
    """differences 5 and 6, an id below last_closed (the unsigned expression wraps: taken), no loop closed yet, no key-frame, a non-zero item status with
    stride 8 and with stride 1, no item status at all"""
    S = 8
    p = Pair(api, S, 4, 8, 6)
    last = [100, 100, -1, 100, 100, 100, 2 ** 40, 0]
    for s in range(S):
        p.load(s, [], None, None, [], None, [], last[s])
    p.check("loaded")
    ids = [105, 106, 0, -1, 110, 99, 2 ** 40 + 6, 5]
    a, st, _ = p.gate(ids, None)
    assert st == [B.SKIPPED, B.TURN, B.TURN, B.IDLE, B.TURN, B.TURN, B.TURN, B.SKIPPED] and a == [0, 1, 1, 0, 1, 1, 1, 0]
    status8 = np.zeros(S * 8, np.int32); status8[8 * 1] = 3; status8[8 * 4] = -1; status8[8 * 2 + 1] = 9          # word 1 of stream 2 is not word 0
    a, st, _ = p.gate(ids, status8, 8)
    assert st == [B.SKIPPED, B.IDLE, B.TURN, B.IDLE, B.IDLE, B.TURN, B.TURN, B.SKIPPED]
    a, st, _ = p.gate(ids, [0, 0, 7, 0, 0, 0, -2, 0], 1)
    assert st == [B.SKIPPED, B.TURN, B.IDLE, B.IDLE, B.TURN, B.TURN, B.IDLE, B.SKIPPED]
    p.check("gates change nothing")


# ---- 2. detect --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 5])
def test_detect_edges_both_copy_paths(api, cap):
    """cap 8: every item of the caller's tables is 16-byte aligned; cap 5: the dword path.  feat_cap 6, K 4, S 3 — twelve streams' worth of edges in four
    calls of three: score equal to the threshold, one ulp below, NaN, +inf, -inf; counts 3 and 4; best_row -1, n[s] and K; a row in range with another
    id; thr_high = +inf"""
    S, K, F = 3, 4, 6
    p = Pair(api, S, K, cap, F)
    _fill(p, [[(3, cap, F), (8, cap - 1, 2), (9, 0, 0)], [(3, 1, 1), (8, cap, F)], [(5, cap, 3), (6, 2, F), (7, cap, F), (2 ** 40, cap - 2, 1)]])
    p.check("loaded")
    below = np.nextafter(THR, np.float32(0))
    w = p.detect([3, 8, 2 ** 40], [0, 1, 3], [THR, below, np.nan], [3, 3, 0], what="thr")
    assert w["status"].tolist() == [0, 1, 0] and w["slot"].tolist() == [0, -1, 3] and w["n_loop"].tolist() == [cap, 0, cap - 2]
    w = p.detect([8, 8, 6], [1, 1, 1], [np.inf, -np.inf, THR], [3, 0, 4], what="inf, cnt 4")
    assert w["status"].tolist() == [0, 1, 1] and w["n_loop"].tolist() == [cap - 1, 0, 0]
    w = p.detect([9, 8, 7], [-1, 2, 4], [0.99] * 3, [0] * 3, what="rows -1, n, K")
    assert w["status"].tolist() == [-1, -1, -1] and w["slot"].tolist() == [-1] * 3
    w = p.detect([9, 3, 6], [2, 1, 2], [0.99] * 3, [0] * 3, what="empty key-frame, row with another id twice")
    assert w["status"].tolist() == [0, -1, -1] and w["n_loop"].tolist() == [0, 0, 0] and w["slot"].tolist() == [2, -1, -1]
    w = p.detect([3, 8, 5], [0, 1, 0], [1.0, np.nan, np.inf], [0, 0, 0], thr_high=np.float32(np.inf), what="+inf threshold")
    assert w["status"].tolist() == [1, 0, 0]
    w = p.detect([3, 8, 5], [0, 1, 0], [0.99] * 3, [3, 2, 3], max_suspected=2, what="max_suspected 2")
    assert w["status"].tolist() == [1, 0, 1]
    p.check("detect changes nothing")


def test_descriptor_pointers_off_a_dword_boundary(api):
    """d_loop_desc one byte past a 16-byte boundary: the descriptors go byte by byte and no byte on either side changes; the same for finish's d_desc"""
    S, K, cap, F = 3, 4, 5, 6
    p = Pair(api, S, K, cap, F)
    _fill(p, [[(3, cap, F)], [(3, 3, 1), (8, cap, F)], [(5, 1, 3)]])
    best_id, best_row = np.array([3, 8, 9], np.uint64), np.array([0, 1, 0], np.int32)
    score, cnt = np.array([0.99, 0.95, 0.99], np.float32), np.zeros(3, np.int32)
    q = [_dev(best_id), _dev(best_row), _dev(score), _dev(cnt)]
    out = p.outputs()
    nbytes = S * cap * 32
    raw = _dev(np.full(nbytes + 16, 0xA5, np.uint8))
    assert raw.data_ptr() % 16 == 0
    p.launch_detect(q, out, desc_ptr=raw.data_ptr() + 1)
    p.sync()
    want = p.ref.detect(best_id, best_row, score, cnt, THR, 3, LS.sentinel_outputs(S, cap, F))
    r = raw.cpu().numpy()
    assert r[1:1 + nbytes].tobytes() == want["desc"].tobytes() and r[0] == 0xA5 and (r[1 + nbytes:] == 0xA5).all()
    for k in KEYS:
        if k != "desc":
            assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert want["status"].tolist() == [0, 0, -1]
    kps, desc, lm = _kfs(77, S, cap, F)
    add, st, _ = p.finish([4, 9, 6], [1, 1, 1], [1, 2, 3], kps, desc, [cap, 3, 1], None, lm, [F, 2, 0], desc_off=1)
    assert st == [B.STORED] * 3
    p.check("put from an odd pointer")


# ---- 3. finish ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 5])
def test_finish_neighbours_refusals_and_clamps(api, cap):
    """confirmed, unconfirmed and idle neighbours in one call; a full stream and an id that does not ascend between good neighbours keep every byte and
    add 0; d_kf_status != 0 stores 0 rows; counts below 0 and above cap are clamped; d_add goes into myslam_lcdbank_append_batch of a bank with the same
    rows per stream, whose ids stay aligned"""
    S, K, F = 5, 4, 6
    p = Pair(api, S, K, cap, F)
    L = api.LoopDatabaseBank(S, K)
    held = [[(1, 1, 1), (2, 2, 2), (3, 3, 3), (4, cap, F)], [(10, cap, F)], [], [(7, 2, 2), (9, 2, 2)], [(1, 1, 1)]]
    _fill(p, held)
    for s, l in enumerate(held):
        if l:
            L.load(s, np.array([x[0] for x in l], np.uint64), R.one_hot([(11 * s + r) % DIM for r in range(len(l))]))
    p.check("loaded")
    descr = _dev(R.one_hot([100 + s for s in range(S)]))
    ast = _sent(S)

    def turn(ids, active, verify, counts, kf_status, nf, seed, what):
        kps, desc, lm = _kfs(seed, S, cap, F)
        add, st, d_add = p.finish(ids, active, verify, kps, desc, counts, kf_status, lm, nf, what=what)
        d_id = _dev(np.asarray(ids, np.uint64))
        L.append_batch(descr.data_ptr(), d_id.data_ptr(), d_add.data_ptr(), ast.data_ptr())
        p.check(what)
        assert ast.cpu().tolist() == [LB.ADDED if a else LB.IDLE for a in add], what
        for s in range(S):
            assert L.get(s)[0].tolist() == p.ref.ids(s), (what, s)
        return add, st

    # full | stored | idle | not ascending (9 <= 9) | confirmed
    add, st = turn([5, 11, 3, 9, 2], [1, 1, 0, 1, 1], [1, 2, 0, 3, 0], [cap, cap + 3, 1, 1, 1], None, [F, F + 2, 1, 1, 1], 1, "mixed")
    assert st == [B.ERR_CAPACITY, B.STORED, B.IDLE, B.ERR_INVALID, B.CLOSED] and add == [0, 1, 0, 0, 0]
    # kf_status != 0: no rows, the table is kept | count below 0 | stored into an empty stream | lower id | stored behind a closed one
    add, st = turn([6, 12, 0, 8, 3], [1, 1, 1, 1, 1], [0, 1, 1, 1, 1], [cap, -4, cap - 1, 1, 2], [0, 0, -3, 0, 0], [F, -1, 3, 1, F], 2, "clamps")
    assert st == [B.CLOSED, B.STORED, B.STORED, B.ERR_INVALID, B.STORED] and add == [0, 1, 1, 0, 1]
    assert p.ref.last_closed == [6, -1, -1, -1, 2] and p.dev.get(2)["rows"].tolist() == [0] and p.dev.get(1)["rows"].tolist() == [cap, cap, 0]
    add, st = turn([7, 13, 1, 10, 4], [0, 1, 1, 1, 1], [1] * 5, [1] * 5, None, [1] * 5, 3, "fills stream 1")
    assert st == [B.IDLE, B.STORED, B.STORED, B.STORED, B.STORED]
    add, st = turn([8, 14, 2, 11, 5], [1] * 5, [1, 1, 1, 1, 1], [1] * 5, None, [1] * 5, 4, "stream 1 full")
    assert st == [B.ERR_CAPACITY, B.ERR_CAPACITY, B.STORED, B.STORED, B.STORED]
    assert api.LoopStoreBank.launches_per_finish() == 2


# ---- 4. links and clear -------------------------------------------------------------------------------------------------------------------
def test_links_stay_in_their_stream_and_clear(api):
    """the store's cases per stream — a pending hit, a stored hit, an id not held, a tag beyond nfeat, a value below -1, no value column — and a list of
    stream 0 that names key-frame 5, which stream 1 holds too: stream 1 keeps every byte"""
    S, K, cap, F = 3, 4, 5, 6
    p = Pair(api, S, K, cap, F)
    _fill(p, [[(5, 2, 4), (9, 1, F)], [(5, 2, 4)], [(4, 0, 3), (5, 1, 2), (6, 1, F)]])
    pending = np.full((S, F), 7, np.int32)
    lists = [[(12, 1, 41), (5, 0, 42), (6, 0, 43), (5, 4, 44), (5, 1, -2), (9, F - 1, -1), (-1, 0, 1), (5, -1, 1)], [], [(6, 0, 3), (12, F, 5), (4, 2, 2 ** 30)]]
    assert p.set_links(lists, pending_ids=[12, 12, 12], pending=pending, what="set") == [3, 0, 2]
    assert pending.tolist() == [[7, 41, 7, 7, 7, 7], [7] * F, [7] * F]
    p.check("set_links")
    assert p.dev.get(1)["lm"][0, :4].tolist() == p.ref.stores[1].kfs[5]["lm"].tolist() and p.dev.get(0)["lm"][0, 0] == 42
    # no value column: clear_links; counts below 0 and above list_cap are clamped; no pending table
    lists = [[(5, 2, -1), (5, 2, -1), (9, 0, -1)], [(5, 1, -1)], [(5, 0, -1)] * 8]
    assert p.set_links(lists, values=False, n=[2, -1, 50], what="clear_links") == [2, 0, 8]
    p.check("clear_links")
    assert p.ref.stores[1].kfs[5]["lm"].tolist() == p.m["lm"][1, 0, :4].tolist() and p.ref.stores[0].kfs[5]["lm"][2] == -1
    p.clear([0, 1, 0])
    p.check("clear")                                                           # a clear moves the count and last_closed and nothing else
    assert p.set_links([[], [(5, 1, 3)], []], what="cleared stream holds nothing") == [0, 0, 0]
    p.check("after clear")


# ---- 5. random histories --------------------------------------------------------------------------------------------------------------------
def _turn_inputs(rng, p, next_id, t):
    S = p.S
    new_id = np.array([(-1 if rng.random() < 0.1 else next_id[s] + int(rng.integers(1, 4))) for s in range(S)], np.int64)
    low = rng.random(S) < 0.05
    for s in range(S):
        ids = p.ref.ids(s)
        if low[s] and ids and new_id[s] >= 0:
            new_id[s] = ids[-1] - int(rng.integers(0, 2))                    # not above the last one held
    status8 = np.zeros(S * 8, np.int32)
    status8[::8] = np.where(rng.random(S) < 0.08, 5, 0); status8[1::8] = 9
    return new_id, status8


def _scan_outputs(rng, p, active):
    """what a scan could have written: mostly a row the stream holds with its id, now and then a row or an id that does not fit"""
    S = p.S
    best_id, best_row = np.zeros(S, np.uint64), np.full(S, -1, np.int32)
    score, cnt = np.zeros(S, np.float32), np.zeros(S, np.int32)
    for s in range(S):
        ids = p.ref.ids(s)
        if not active[s] or not ids:
            continue
        r = int(rng.integers(0, len(ids)))
        best_id[s], best_row[s] = ids[r], r
        score[s] = rng.choice(np.array([0.5, 0.94, 0.95, 0.99, np.nan], np.float32), p=[0.2, 0.2, 0.3, 0.2, 0.1])
        cnt[s] = rng.integers(0, 5)
        k = rng.random()
        if k < 0.05:
            best_row[s] = len(ids)
        elif k < 0.1:
            best_id[s] += 1
    return best_id, best_row, score, cnt


@pytest.mark.parametrize("S", [1, 3, 65])
def test_random_histories_in_lock_step(api, S):
    """40 turns of gate -> detect -> finish -> lcdbank append, K 6, cap 5 (odd: both copy paths), verify statuses and scan outputs drawn here, a clear of
    random streams now and then: the model and the device are equal after every call, and the loop database bank holds the same ids at the same rows"""
    rng = np.random.default_rng(300 + S)
    K, cap, F = 6, 5, 6
    p = Pair(api, S, K, cap, F, every_get=S <= 3)
    L = api.LoopDatabaseBank(S, K)
    descr = _dev(R.one_hot([(7 * s) % DIM for s in range(S)]))
    ast = _sent(S)
    next_id = [0] * S
    seen = set()
    for t in range(40):
        new_id, status8 = _turn_inputs(rng, p, next_id, t)
        active, gst, d_active = p.gate(new_id, status8, 8, what=("gate", t))
        best_id, best_row, score, cnt = _scan_outputs(rng, p, active)
        w = p.detect(best_id, best_row, score, cnt, what=("detect", t))
        verify = [B.VERIFY_CONFIRMED if (w["status"][s] == B.CANDIDATE and rng.random() < 0.3) else int(rng.integers(1, 4)) for s in range(S)]
        kps, desc, lm = _kfs(1000 * S + t, S, cap, F)
        counts, nf = rng.integers(-1, cap + 2, S), rng.integers(-1, F + 2, S)
        kf_status = None if t % 3 == 0 else np.where(rng.random(S) < 0.1, -3, 0)
        cur = np.where(new_id >= 0, new_id, 0).astype(np.uint64)
        add, fst, d_add = p.finish(cur, active, verify, kps, desc, counts, kf_status, lm, nf, what=("finish", t))
        d_id = _dev(cur)
        L.append_batch(descr.data_ptr(), d_id.data_ptr(), d_add.data_ptr(), ast.data_ptr())
        p.check(("turn", t), gets=None if S <= 3 else t % 13 == 12)
        assert ast.cpu().tolist() == [LB.ADDED if a else LB.IDLE for a in add], t
        for s in range(S):
            if new_id[s] >= 0:
                next_id[s] = max(next_id[s], int(new_id[s]))
        seen |= set(gst) | set(fst) | {10 + int(x) for x in w["status"]}
        if t % 7 == 6:
            flags = (rng.random(S) < 0.4).astype(np.int32)
            p.clear(flags)
            d_f = _dev(flags)
            L.clear_batch(d_f.data_ptr())
            for s in range(S):
                if flags[s]:
                    next_id[s] = 0
            p.check(("clear", t), gets=False)
    p.check("end", gets=True)
    for s in range(S):
        assert L.get(s)[0].tolist() == p.ref.ids(s), s
    if S >= 3:
        assert seen >= {B.TURN, B.SKIPPED, B.IDLE, B.CLOSED, B.STORED, 10 + B.CANDIDATE, 10 + B.NO_LOOP}, seen
    if S == 65:
        assert seen >= {B.ERR_CAPACITY, B.ERR_INVALID, 10 + B.ERR_INVALID}, seen


# ---- 6. against the single store -------------------------------------------------------------------------------------------------------------
def test_same_answers_as_single_stores(api):
    """S = 3, a history without a closed loop: every key-frame the bank stores is put into one api.LoopKeyFrameStore per stream as well
    (put_batch(batch = 1)); detect_batch(nq = 1) of each store writes the bytes the bank's detect writes for that stream"""
    import torch
    S, K, cap, F = 3, 6, 5, 6
    rng = np.random.default_rng(8)
    p = Pair(api, S, K, cap, F)
    stores = [api.LoopKeyFrameStore(K, cap, F) for _ in range(S)]
    for t in range(5):
        ids = np.array([10 * t + s + (1 if t else 0) for s in range(S)], np.int64)
        active, _, _ = p.gate(ids, None)
        active[t % S] = 0                                                      # one stream sits every turn out
        kps, desc, lm = _kfs(400 + t, S, cap, F)
        counts, nf = rng.integers(-1, cap + 2, S).astype(np.int32), rng.integers(-1, F + 2, S).astype(np.int32)
        kf_status = np.array([0, -3 if t == 2 else 0, 0], np.int32)
        add, st, _ = p.finish(ids, active, [1 + t % 3] * S, kps, desc, counts, kf_status, lm, nf)
        assert st == [B.STORED if a else B.IDLE for a in active]
        d = [_dev(kps), _dev(desc), _dev(counts), _dev(kf_status), _dev(lm), _dev(nf)]
        for s in range(S):
            if add[s]:
                stores[s].put_batch([int(ids[s])], d[0].data_ptr() + s * cap * 28, d[1].data_ptr() + s * cap * 32, d[2].data_ptr() + 4 * s,
                                    d[3].data_ptr() + 4 * s, d[4].data_ptr() + s * F * 4, d[5].data_ptr() + 4 * s)
        torch.cuda.synchronize()
        assert [len(x) for x in stores] == p.ref.sizes()
        for trial in range(3):
            best_id, best_row, score, cnt = _scan_outputs(rng, p, [1] * S)
            best_id = np.array([p.ref.ids(s)[best_row[s]] if 0 <= best_row[s] < len(p.ref.ids(s)) else 4 for s in range(S)], np.uint64)      # ids a store holds too
            w = p.detect(best_id, best_row, score, cnt, what=("bank", t, trial))
            out = p.outputs()
            q = [_dev(best_id), _dev(score), _dev(cnt)]
            for s in range(S):
                stores[s].detect_batch(q[0].data_ptr() + 8 * s, q[1].data_ptr() + 4 * s, q[2].data_ptr() + 4 * s, 1, out["desc"].data_ptr() + s * cap * 32,
                                       out["n_loop"].data_ptr() + 4 * s, out["pyr"].data_ptr() + s * cap * 28, out["lm"].data_ptr() + s * F * 4,
                                       out["slot"].data_ptr() + 4 * s, out["status"].data_ptr() + 4 * s)
            torch.cuda.synchronize()
            for k in KEYS:
                assert out[k].cpu().numpy().tobytes() == w[k].tobytes(), (t, trial, k)


# ---- 7. recorded -------------------------------------------------------------------------------------------------------------------------------
def test_recorded_turn_replays_over_its_own_puts(api):
    """gate -> lcdbank query -> detect -> finish -> lcdbank append recorded ONCE into a StepGraph and replayed 9 times with the device inputs rewritten in
    between: each replay equals the two models, the key-frames stored and the rows appended by earlier replays included.  The image descriptor of
    key-frame id is one-hot at column id; a query that scores 0.95 on an earlier key-frame of its stream makes a candidate"""
    import torch
    S, K, cap, F, MIN = 3, 8, 5, 6, 1
    rng = np.random.default_rng(12)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sp = stream.cuda_stream
        p = Pair(api, S, K, cap, F, stream=sp)
        L = api.LoopDatabaseBank(S, K, sp)
        Lref = LB.Bank(S, K)
        d_new = _dev(np.full(S, -1, np.int64)); d_q = _dev(np.zeros((S, DIM), np.float32)); d_descr = _dev(np.zeros((S, DIM), np.float32))
        d_ver = _dev(np.ones(S, np.int32))
        kin = [_dev(np.zeros((S, cap), LS.KP_DTYPE)), _dev(np.zeros((S, cap, 32), np.uint8)), _dev(np.zeros(S, np.int32)), _dev(np.zeros((S, F), np.int32)),
               _dev(np.zeros(S, np.int32))]
        d_act, gst, add, fst, ast, qst = (_sent(S) for _ in range(6))
        scan = [_dev(np.zeros(S, np.uint64)), _dev(np.zeros(S, np.float32)), _sent(S), _sent(S)]          # best id, score, cnt, row
        out = p.outputs()

        def body():
            p.dev.gate_batch(d_new.data_ptr(), 0, 1, d_act.data_ptr(), gst.data_ptr())
            L.query_batch(d_q.data_ptr(), d_new.data_ptr(), d_act.data_ptr(), scan[0].data_ptr(), scan[1].data_ptr(), scan[2].data_ptr(), scan[3].data_ptr(),
                          qst.data_ptr(), thr_low=float(R.THR), min_size=MIN)
            p.launch_detect([scan[0], scan[3], scan[1], scan[2]], out)
            p.dev.finish_batch(d_new.data_ptr(), d_act.data_ptr(), d_ver.data_ptr(), kin[0].data_ptr(), kin[1].data_ptr(), kin[2].data_ptr(), 0,
                               kin[3].data_ptr(), kin[4].data_ptr(), add.data_ptr(), fst.data_ptr())
            L.append_batch(d_descr.data_ptr(), d_new.data_ptr(), add.data_ptr(), ast.data_ptr())

        g = api.StepGraph.record(sp, [], body)
        assert g.node_count() == 1 + api.LoopDatabaseBank.launches_per_query() + 1 + api.LoopStoreBank.launches_per_finish() + 1
        torch.cuda.synchronize()
        p.check("recording ran nothing")
        next_id = [0, 40, 80]
        seen = set()
        for t in range(9):
            # 25 apart: the scan's cut-off window holds no earlier id; 3 apart every third turn: inside the five behind a loop closed the turn before
            new_id = np.array([next_id[s] + (0 if t == 0 else 3 if t % 3 == 1 else 25) for s in range(S)], np.int64)
            if t == 4:
                new_id[1] = -1
            q = np.zeros((S, DIM), np.float32)
            for s in range(S):
                ids = p.ref.ids(s)
                if ids:
                    q[s, ids[int(rng.integers(0, len(ids)))] % DIM] = (0.95, 0.5, 0.95)[(t + s) % 3]
            descr = R.one_hot([int(i) % DIM if i >= 0 else 0 for i in new_id])
            verify = np.array([B.VERIFY_CONFIRMED if (t + s) % 4 == 3 else 1 + (t + s) % 3 for s in range(S)], np.int32)
            kps, desc, lm = _kfs(700 + t, S, cap, F)
            counts, nf = rng.integers(0, cap + 1, S).astype(np.int32), rng.integers(0, F + 1, S).astype(np.int32)
            for dst, src in ((d_new, new_id), (d_q, q), (d_descr, descr), (d_ver, verify), (kin[0], kps), (kin[1], desc), (kin[2], counts), (kin[3], lm), (kin[4], nf)):
                dst.copy_(_dev(src))
            for k, v in p.outputs().items():
                out[k].copy_(v)
            for x in (d_act, gst, add, fst, ast, qst, scan[2], scan[3]):
                x.fill_(SENT)
            g.launch(sp)
            torch.cuda.synchronize()
            active, wg = p.ref.gate(new_id)
            assert (d_act.cpu().tolist(), gst.cpu().tolist()) == (active, wg), t
            cur = new_id.astype(np.uint64)
            e = LB.as_arrays(Lref.query(q, cur, active, R.THR, MIN))
            got = (scan[0].cpu().numpy().view(np.uint64), scan[1].cpu().numpy(), scan[2].cpu().numpy(), scan[3].cpu().numpy(), qst.cpu().numpy())
            for a, b in zip(got, e):
                assert a.tobytes() == np.asarray(b, a.dtype).tobytes(), t
            want = p.ref.detect(e[0], e[3], e[1], e[2], THR, 3, LS.sentinel_outputs(S, cap, F))
            for k in KEYS:
                assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), (t, k)
            n0 = p.ref.sizes()
            wadd, wst = p.ref.finish(cur, active, verify, kps, desc, counts, None, lm, nf)
            p.note_finish(n0, wst, cur, kps, desc, counts, None, lm, nf)
            assert (add.cpu().tolist(), fst.cpu().tolist()) == (wadd, wst), t
            assert ast.cpu().tolist() == Lref.append(descr, cur, wadd), t
            p.check(("replay", t))
            for s in range(S):
                if new_id[s] >= 0:
                    next_id[s] = int(new_id[s])
                assert L.get(s)[0].tolist() == p.ref.ids(s) == Lref.ids[s], (t, s)
            seen |= set(wg) | set(wst) | {10 + int(x) for x in want["status"]}
        assert seen >= {B.TURN, B.SKIPPED, B.IDLE, B.CLOSED, B.STORED, 10 + B.CANDIDATE, 10 + B.NO_LOOP}, seen
        assert sum(p.ref.sizes()) >= 9


# ---- 8. the real chain ---------------------------------------------------------------------------------------------------------------------------
def test_chain_for_two_streams(api, synth):
    """S = 2 on the synthetic key-frames of tests/test_gpu_loop_store.py: gate -> lcdbank query -> bank detect -> loop_match_batch -> verify_batch -> finish
    -> lcdbank append enqueued on one stream with no host read in between.  Stream 0's query resembles key-frame 1 and is confirmed: nothing is stored,
    last_closed moves and the next five key-frames are skipped.  Stream 1's resembles key-frame 3, which keeps nine map points: too few, so the current
    key-frame is stored and appended."""
    import torch
    from test_gpu_loop_store import CH_CAP, CH_FEAT, CH_IDS, CH_LAND, CH_OUT, chain_scene, chain_store_inputs
    db, kfs, pos, Kc, q5 = chain_scene(synth)
    S, K, cap, F, OUT = 2, 8, CH_CAP, CH_FEAT, CH_OUT
    hit = [1, 3]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sp = stream.cuda_stream
        p = Pair(api, S, K, cap, F, stream=sp)
        L = api.LoopDatabaseBank(S, K, sp)
        kps, desc, counts, lm, nf = chain_store_inputs(kfs)
        for s in range(S):
            p.load(s, CH_IDS, kps, desc, counts, lm, nf)
            L.load(s, np.asarray(CH_IDS, np.uint64), db)
        solver = api.PnPSolver(S, OUT, 100, stream=sp)
        q = np.stack([q5[0], q5[2]])
        cd = np.full((S, cap, 32), 0xFF, np.uint8); cp = np.frombuffer(b"\xff" * (S * cap * 28), LS.KP_DTYPE).reshape(S, cap).copy()
        nc = np.zeros(S, np.int32); xy = np.full((S, F, 2), np.nan, np.float32)
        for b, k in enumerate(hit):
            kf = kfs[k]
            n = len(kf["cur_cls"])
            cd[b, :n] = kf["cur_desc"]; cp[b, :n] = 0; cp["class_id"][b, :n] = kf["cur_cls"]; nc[b] = n; xy[b, :len(kf["uv"])] = kf["uv"]
        cur_lm = np.random.default_rng(5).integers(-1, CH_LAND, (S, F)).astype(np.int32)
        cur_nf = np.array([F, F - 3], np.int32)
        t_cd, t_cp, t_nc, t_xy, t_pos, t_q = _dev(cd), _dev(cp), _dev(nc), _dev(xy), _dev(pos), _dev(q)
        t_lm, t_nf = _dev(cur_lm), _dev(cur_nf)
        new_id = np.array([200, 200], np.int64)
        d_new = _dev(new_id)
        z = lambda *sh, dt=torch.int32: torch.full(sh, -7, dtype=dt, device="cuda")
        d_act, gst, add, fst, ast, qst = (_sent(S) for _ in range(6))
        scan = [z(S, dt=torch.int64), z(S, dt=torch.float32), z(S), z(S)]
        loop = p.outputs()
        m = dict(ti=z(S, cap), dist=z(S, cap), pairs=z(S, cap, 2), np=z(S), valid=z(S, OUT, 2), p3=z(S, OUT, 3, dt=torch.float32), p2=z(S, OUT, 2, dt=torch.float32),
                 cnt=z(S), st=z(S))
        v = dict(pose=torch.full((S, 7), 0.25, dtype=torch.float64, device="cuda"), flag=torch.full((S, OUT), 255, dtype=torch.uint8, device="cuda"), ninl=z(S), st=z(S))
        # the device chain: seven enqueues, nothing read in between
        p.dev.gate_batch(d_new.data_ptr(), 0, 1, d_act.data_ptr(), gst.data_ptr())
        L.query_batch(t_q.data_ptr(), d_new.data_ptr(), d_act.data_ptr(), scan[0].data_ptr(), scan[1].data_ptr(), scan[2].data_ptr(), scan[3].data_ptr(),
                      qst.data_ptr(), min_size=2)
        p.launch_detect([scan[0], scan[3], scan[1], scan[2]], loop)
        api.loop_match_batch(loop["desc"].data_ptr(), loop["n_loop"].data_ptr(), t_cd.data_ptr(), t_nc.data_ptr(), loop["pyr"].data_ptr(), t_cp.data_ptr(),
                             S, cap, t_xy.data_ptr(), loop["lm"].data_ptr(), F, t_pos.data_ptr(), 0, CH_LAND, 10, OUT, m["ti"].data_ptr(),
                             m["dist"].data_ptr(), m["pairs"].data_ptr(), m["np"].data_ptr(), m["valid"].data_ptr(), m["p3"].data_ptr(),
                             m["p2"].data_ptr(), m["cnt"].data_ptr(), m["st"].data_ptr(), sp)
        solver.verify_batch(m["p3"].data_ptr(), m["p2"].data_ptr(), m["cnt"].data_ptr(), S, Kc, v["pose"].data_ptr(), v["flag"].data_ptr(),
                            v["ninl"].data_ptr(), v["st"].data_ptr())
        p.dev.finish_batch(d_new.data_ptr(), d_act.data_ptr(), v["st"].data_ptr(), t_cp.data_ptr(), t_cd.data_ptr(), t_nc.data_ptr(), 0, t_lm.data_ptr(),
                           t_nf.data_ptr(), add.data_ptr(), fst.data_ptr())
        L.append_batch(t_q.data_ptr(), d_new.data_ptr(), add.data_ptr(), ast.data_ptr())
        torch.cuda.synchronize()
        assert d_act.cpu().tolist() == [1, 1] and qst.cpu().tolist() == [LB.SCANNED] * 2
        best, row = scan[0].cpu().numpy().view(np.uint64), scan[3].cpu().numpy()
        assert best.tolist() == [CH_IDS[1], CH_IDS[3]] and row.tolist() == hit
        want = p.ref.detect(best, row, scan[1].cpu().numpy(), scan[2].cpu().numpy(), THR, 3, LS.sentinel_outputs(S, cap, F))
        for k in KEYS:
            assert loop[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert want["status"].tolist() == [0, 0] and want["slot"].tolist() == hit
        verify = v["st"].cpu().tolist()
        assert verify == [api.VERIFY_CONFIRMED, api.VERIFY_FEW_MATCHES] and m["cnt"].cpu().tolist()[1] == 9
        n0 = p.ref.sizes()
        wadd, wst = p.ref.finish(new_id.astype(np.uint64), [1, 1], verify, cp, cd, nc, None, cur_lm, cur_nf)
        p.note_finish(n0, wst, new_id, cp, cd, nc, None, cur_lm, cur_nf)
        assert (add.cpu().tolist(), fst.cpu().tolist()) == (wadd, wst) == ([0, 1], [B.CLOSED, B.STORED])
        assert ast.cpu().tolist() == [LB.IDLE, LB.ADDED]
        p.check("chain")
        assert p.ref.last_closed == [200, -1] and p.ref.sizes() == [6, 7]
        for s in range(S):
            assert L.get(s)[0].tolist() == p.ref.ids(s), s
        for kf_id in range(201, 208):                                          # the five behind the closed loop
            _, st, _ = p.gate([kf_id, kf_id])
            assert st == [B.SKIPPED if kf_id <= 205 else B.TURN, B.TURN], kf_id


# ---- 9. limits and errors ---------------------------------------------------------------------------------------------------------------------------
def test_limit_shape(api):
    """cap 16384 and feat_cap 65536, the matcher's limits, S 1, K 2: one put and one detect of a full key-frame"""
    cap, F = 16384, 65536
    p = Pair(api, 1, 2, cap, F, every_get=False)
    kps, desc, lm = _kfs(11, 1, cap, F)
    add, st, _ = p.finish([2 ** 62], [1], [1], kps, desc, [cap], [0], lm, [F])
    assert st == [B.STORED]
    w = p.detect([2 ** 62], [0], [0.99], [1])
    assert w["status"].tolist() == [0] and w["n_loop"].tolist() == [cap] and w["pyr"].tobytes() == kps.tobytes() and w["lm"].tobytes() == lm.tobytes()
    assert p.detect([2 ** 62], [1], [0.99], [1])["status"].tolist() == [-1]
    p.check("limit", gets=True)


def test_call_level_errors(api):
    """nothing is enqueued, and the bank answers as before"""
    import ctypes as C
    import torch
    S, K, cap, F = 2, 3, 5, 6
    INV, CAPY = api.ERR_INVALID, api.ERR_CAPACITY
    for args, code in (((0, K, cap, F), INV), ((S, 0, cap, F), INV), ((S, K, 0, F), INV), ((S, K, cap, -1), INV), ((S, K, 16385, F), CAPY),
                       ((S, K, cap, 65537), CAPY), ((65536, K, cap, F), CAPY)):
        with pytest.raises(api.MyslamError) as err:
            api.LoopStoreBank(*args)
        assert err.value.code == code, args
    p = Pair(api, S, K, cap, F)
    _fill(p, [[(3, cap, F), (8, 2, 2)], [(5, 1, 1)]])
    p.check("loaded")
    kps, desc, lm = _kfs(9, 4, cap, F)
    ld = lambda s, ids, rows, nf, last=-1: _code(api, p.dev.load, s, ids, kps[:len(ids)], desc[:len(ids)], rows, lm[:len(ids)], nf, last)
    assert ld(0, [4, 4], [1, 1], [1, 1]) == INV and ld(0, [5, 4], [1, 1], [1, 1]) == INV and ld(0, [1, 2, 3, 4], [1] * 4, [1] * 4) == CAPY
    assert ld(0, [4], [cap + 1], [1]) == INV and ld(0, [4], [-1], [1]) == INV and ld(0, [4], [1], [F + 1]) == INV and ld(0, [4], [1], [1], -2) == INV
    assert ld(2, [4], [1], [1]) == INV and ld(-1, [4], [1], [1]) == INV
    p.check("refused loads")
    out = p.outputs()
    a8 = _dev(np.zeros(S, np.uint64)); a4 = _dev(np.zeros(S, np.int32)); f4 = _dev(np.zeros(S, np.float32)); i1, i2 = _sent(S), _sent(S)
    good = [a8.data_ptr(), a4.data_ptr(), f4.data_ptr(), a4.data_ptr(), out["desc"].data_ptr(), out["n_loop"].data_ptr(), out["pyr"].data_ptr(),
            out["lm"].data_ptr(), out["slot"].data_ptr(), out["status"].data_ptr()]
    for k in range(10):
        assert _code(api, p.dev.detect_batch, *(good[:k] + [0] + good[k + 1:])) == INV, k
    gg = [a8.data_ptr(), 0, 1, i1.data_ptr(), i2.data_ptr()]
    for k in (0, 3, 4):
        assert _code(api, p.dev.gate_batch, *(gg[:k] + [0] + gg[k + 1:])) == INV, k
    assert _code(api, p.dev.gate_batch, a8.data_ptr(), a4.data_ptr(), 0, i1.data_ptr(), i2.data_ptr()) == INV      # an item status needs a stride
    t = [_dev(kps[:S]), _dev(desc[:S]), _dev(lm[:S])]
    gf = [a8.data_ptr(), a4.data_ptr(), a4.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), a4.data_ptr(), 0, t[2].data_ptr(), a4.data_ptr(), i1.data_ptr(), i2.data_ptr()]
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10):
        assert _code(api, p.dev.finish_batch, *(gf[:k] + [0] + gf[k + 1:])) == INV, k
    l8 = _dev(np.zeros((S, 4), np.int64)); l4 = _dev(np.zeros((S, 4), np.int32))
    gl = [l8.data_ptr(), l4.data_ptr(), 0, a4.data_ptr(), 4, 0, 0, 0]
    for k in (0, 1, 3):
        assert _code(api, p.dev.set_links_batch, *(gl[:k] + [0] + gl[k + 1:])) == INV, k
    assert _code(api, p.dev.set_links_batch, *(gl[:4] + [0] + gl[5:])) == INV                                        # list_cap 0
    assert _code(api, p.dev.set_links_batch, *(gl[:5] + [a8.data_ptr(), 0, 0])) == INV                                # a pending id without its table
    assert _code(api, p.dev.clear_batch, 0) == INV
    lib = api.lib()
    assert lib.myslam_loop_bank_sizes(p.dev._h, None) == INV and lib.myslam_loop_bank_view(p.dev._h, None) == INV
    n = C.c_int()
    assert lib.myslam_loop_bank_get(p.dev._h, 0, None, None, None, None, None, None, 1, C.byref(n), None) == INV
    last = C.c_int64()
    assert lib.myslam_loop_bank_get(p.dev._h, 0, None, None, None, None, None, None, 1, C.byref(n), C.byref(last)) == CAPY and n.value == 2
    assert lib.myslam_loop_bank_get(p.dev._h, S, None, None, None, None, None, None, 4, C.byref(n), C.byref(last)) == INV
    torch.cuda.synchronize()
    fresh = LS.sentinel_outputs(S, cap, F)
    assert all(out[k].cpu().numpy().tobytes() == fresh[k].tobytes() for k in KEYS) and i1.cpu().tolist() == [SENT] * S == i2.cpu().tolist()
    p.check("refused calls")
    # load / get / sizes refuse a stream that is being recorded, and the recording goes on
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p.dev.set_stream(stream.cuda_stream)
        refused = []

        def body():
            refused.append(ld(1, [9], [1], [1]))
            refused.append(_code(api, p.dev.get, 0))
            refused.append(_code(api, p.dev.sizes))
            p.dev.gate_batch(a8.data_ptr(), 0, 1, i1.data_ptr(), i2.data_ptr())

        g = api.StepGraph.record(stream.cuda_stream, [], body)
        assert refused == [api.ERR_UNSUPPORTED] * 3 and g.node_count() == 1
        torch.cuda.synchronize()
    p.check("after the recording")


# ---- 10. facade ---------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_facade_bank(api, tmp_path):
    """myslam::LoopKeyFrameStoreBank (host/myslam_hip.hpp) in a compiled host program: tests/cpp/loop_bank_test.cpp against the literal statements of
    InsertNewKeyFrame and LoopClosingRun"""
    from conftest import PKG_DIR, ROOT
    exe = str(tmp_path / "loop_bank_test")
    cmd = ["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "loop_bank_test.cpp"), "-o", exe,
           "-L" + PKG_DIR, "-lmyslam_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "LOOP BANK TEST OK" in r.stdout, r.stdout + r.stderr
