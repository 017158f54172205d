"""Link upkeep on the device (include/myslam_hip.h, LINK UPKEEP): the culled list of myslam_backend_optimize_batch's write-back,
myslam_loop_store_clear_links_batch, myslam_map_filter_landmarks_batch and myslam_tracker_clear_links_batch against the plain-Python rules of
tests/link_upkeep_ref.py (pinned to the object model of the reference's Map by tests/test_link_upkeep_ref.py), and the same histories on the device
with the device's own solve: after every event the gathered and filtered table of every stored key-frame is the model's."""
import numpy as np
import pytest

import backend_ref as br
import link_upkeep_ref as lu
import loop_store_ref as R
import map_insert_ref as mi
import test_whole_map_model as T
import tracker_cases as TC
import tracker_kf_cases as KC
import whole_map_model as wm
from test_gpu_backend import Run as BeRun, caps_of, check_against_walk
from test_gpu_loop_store import FIVE_IDS, _dev, five
from test_gpu_map_archive import Dev
from test_gpu_map_insert import OUT_FILL, TABLE_ARGS, Run as InsRun
from test_gpu_tracker_init import InitRig, pair
from test_gpu_tracker_kf import STATE_KEYS, Rig, _same, _state_bytes

pytestmark = pytest.mark.gpu

NEG_INF = np.float32(-np.inf)
INT_MIN = -2 ** 31


class DevArray:
    """a device pointer of a handle's view as something torch can wrap (the CUDA array interface)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


def culled_tensors(h, B, obs_cap):
    """Backend.culled_view() as torch tensors over the handle's own memory: (kf ids [B, obs_cap] i64, tags [B, obs_cap] i32, counts [B] i32)"""
    import torch
    kf, tag, n = h.culled_view()
    return (torch.as_tensor(DevArray(kf, (B, obs_cap), "<i8"), device="cuda"), torch.as_tensor(DevArray(tag, (B, obs_cap), "<i4"), device="cuda"),
            torch.as_tensor(DevArray(n, (B,), "<i4"), device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the culled list against obs_report

def fixed_points_map(K, n_obs, culls):
    """one free key-frame (id 40) seeing n landmarks whose front row is of a key-frame that left (fixed landmarks: two rows each, the ACTIVE one second),
    the last landmark with a third row when n_obs is odd; the landmarks in `culls` are seen 80 px off (a fixed landmark cannot follow: the edge fails)"""
    n = n_obs // 2
    rng = np.random.default_rng(n_obs)
    m = br.Map(); m.kfs[40] = np.array([0, 0, 0, 1, 0, 0, 0.0])
    tag = 0
    for j in range(n):
        pos = np.array([rng.uniform(-3, 3), rng.uniform(-1, 1), rng.uniform(8, 20)])
        uv = np.array([K[0] * pos[0] / pos[2] + K[2], K[1] * pos[1] / pos[2] + K[3]])
        mp = br.MapPoint(100 + 2 * j, pos)
        mp.obs.append(br.Obs(33, uv[0] + 1.0, uv[1], False, tag)); tag += 1
        o = br.Obs(40, uv[0] + (80.0 if j in culls else 0.0), uv[1] - (80.0 if j in culls else 0.0), False, tag); tag += 1
        mp.obs.append(o); mp.active_obs.append(o)
        if j == n - 1 and n_obs % 2:
            mp.obs.append(br.Obs(35, uv[0], uv[1] + 1.0, False, tag)); tag += 1
        m.mps[mp.id] = mp
    assert len(br.rows_of(m)) == n_obs
    return m


def test_culled_view_is_obs_report_in_row_order(api, synth):
    import torch
    made = [br.make_map(synth, s, n_kf=6, n_mp=60) for s in (0x300, 0x301)]
    K = made[0][1]
    # rows that end one below, on and one above a multiple of the write-back's 512-row chunk, culls on both sides of row 512 (landmark j's edge is row 2j + 1)
    chunked = [fixed_points_map(K, n, culls=(3, 254, 255, 256, 257, n // 2 - 1)) for n in (1023, 1024, 1025)]
    edgeless = made[1][0].clone()                                           # EMPTY: every edge row carries OUTLIER or belongs to an outlier point
    for k, mp in enumerate(edgeless.mps.values()):
        if k % 2:
            mp.outlier = True
        else:
            for o in mp.active_obs:
                o.outlier = True
    maps = [made[0][0], made[1][0]] + chunked + [edgeless, made[0][0].clone()]
    B, spare = len(maps), 2                                                 # two more items in the handle than in the call
    caps = caps_of(maps)
    t = br.pack_batch(maps, *caps)
    t["n_obs"][B - 1] = -3                                                  # refused
    h = api.Backend(B + spare, *caps)
    kf, tag, n = culled_tensors(h, B + spare, caps[2])
    assert n.cpu().numpy().tolist() == [0] * (B + spare)                    # before the first call: empty lists
    kf.fill_(-4242); tag.fill_(-4343); n.fill_(-4444)
    torch.cuda.synchronize()
    r = BeRun(api, t, K, caps, handle=h)
    out = r()
    assert out["status"].tolist() == [br.DONE] * 5 + [br.EMPTY, br.INVALID]
    check_against_walk(r, r.host, out, maps[:5])                            # every existing output of the call, as before
    gk, gt, gn = kf.cpu().numpy(), tag.cpu().numpy(), n.cpu().numpy()
    for b in range(B):
        n_obs = max(int(r.host["n_obs"][b]), 0)
        rows = np.nonzero(out["obs_report"][b, :n_obs] == 1)[0] if out["status"][b] == br.DONE else np.zeros(0, int)
        want = [(int(r.host["kf_id"][b, r.host["obs_kf"][b, x]]), int(r.host["obs_tag"][b, x])) for x in rows]
        assert gn[b] == len(want) == out["n_out"][b], b
        assert list(zip(gk[b, :gn[b]].tolist(), gt[b, :gn[b]].tolist())) == want, b
        assert (gk[b, gn[b]:] == -4242).all() and (gt[b, gn[b]:] == -4343).all()          # (unspecified by the contract; the kernel writes none of them)
        assert want == lu.culled_list({k: r.host[k][b] for k in ("kf_id", "obs_kf", "obs_tag")} | {"obs_mp": r.host["obs_mp"][b, :n_obs]}, out["obs_report"][b])
    assert gn[0] > 0 and gn[1] > 0 and gn[B - 2:B].tolist() == [0, 0]
    for b in (2, 3, 4):
        rows = np.nonzero(out["obs_report"][b] == 1)[0]
        assert (rows < 512).any() and (rows >= 512).any() and 511 in rows and 513 in rows, (b, rows)
    assert (gk[B:] == -4242).all() and (gt[B:] == -4343).all() and (gn[B:] == -4444).all()      # items beyond the call's batch keep their bytes
    # an item's list does not depend on its slot or its neighbours
    h2 = api.Backend(3, *caps)
    r2 = BeRun(api, br.pack_batch([maps[3], maps[0], maps[1]], *caps), K, caps, handle=h2)
    r2()
    k2, t2, n2 = (x.cpu().numpy() for x in culled_tensors(h2, 3, caps[2]))
    for a, b in ((0, 3), (1, 0), (2, 1)):
        assert n2[a] == gn[b] and _same(k2[a, :n2[a]], gk[b, :gn[b]]) and _same(t2[a, :n2[a]], gt[b, :gn[b]])
    # recorded: the list is part of the three launches
    assert h.launches_per_call() == 3
    r.restore(); kf.fill_(-1); tag.fill_(-1); n.fill_(-1)
    torch.cuda.synchronize()
    g = api.StepGraph.record(r.stream.cuda_stream, [], r.enqueue)
    r.restore()
    r.stream.wait_stream(torch.cuda.current_stream())
    g.launch(r.stream.cuda_stream)
    r.stream.synchronize()
    assert _same(n.cpu().numpy()[:B], gn[:B]) and all(_same(kf.cpu().numpy()[b, :gn[b]], gk[b, :gn[b]]) and _same(tag.cpu().numpy()[b, :gn[b]], gt[b, :gn[b]])
                                                      for b in range(B))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. clear_links against the Python rule

def ref_store(p):
    """tests/link_upkeep_ref.Store with the landmark tables of a test_gpu_loop_store.Pair's restatement (shared arrays: a clear shows in both)"""
    s = lu.Store(p.feat_cap)
    for kf_id, kf in p.ref.kfs.items():
        s.ids.append(int(kf_id)); s.tables.append(kf["lm"])
    return s


def clear(api, p, lists, n=None, list_cap=8, pending=None, batch=None, with_count=True):
    """one clear_links_batch on the Pair's device store and the rule on its restatement.  lists: per item [(kf id, tag)]; n: the device-side counts;
    pending: (ids per item, table [B, feat_cap]) or None.  -> (device counts, device pending table)"""
    import torch
    B = len(lists)
    ids = np.full((B, list_cap), -77, np.int64); tags = np.full((B, list_cap), -78, np.int32)
    for b, l in enumerate(lists):
        for j, (k, t) in enumerate(l):
            ids[b, j], tags[b, j] = k, t
    n = np.array([len(l) for l in lists] if n is None else n, np.int32)
    d = [_dev(ids), _dev(tags), _dev(n)]
    d_cnt = torch.full((B + 1,), -99, dtype=torch.int32, device="cuda")
    d_pid = d_tab = None
    if pending is not None:
        d_pid, d_tab = _dev(np.asarray(pending[0], np.int64)), _dev(np.asarray(pending[1], np.int32))
    torch.cuda.synchronize()
    p.dev.clear_links_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), list_cap, B if batch is None else batch,
                            d_pid.data_ptr() if pending is not None else None, d_tab.data_ptr() if pending is not None else None,
                            d_cnt.data_ptr() if with_count else None)
    torch.cuda.synchronize()
    s = ref_store(p)
    tab = None if pending is None else np.array(pending[1], np.int32)
    want = [s.clear_links(lists[b] + [(-77, -78)] * list_cap, n=n[b], list_cap=list_cap, pending_id=None if pending is None else int(pending[0][b]),
                          pending=None if pending is None else tab[b]) for b in range(B)]
    got = d_cnt.cpu().numpy()
    assert got[B] == -99 and (got[:B].tolist() == want if with_count else (got == -99).all()), (got, want)
    if pending is not None:
        assert _same(d_tab.cpu().numpy(), tab)
    return want, tab


def whole_store(p, extra_ids=()):
    """every key-frame held, gathered with thr_high = -inf on sentinel-filled outputs and compared WHOLE with the restatement -> its bytes"""
    ids = list(p.ref.kfs) + list(extra_ids)
    return p.detect(ids, [0.5] * len(ids), [0] * len(ids), thr_high=NEG_INF)[0]


def test_clear_links_is_the_rule_and_touches_nothing_else(api):
    cap, F = 37, 16
    p = five(api, cap)                                                      # stored feature counts 0, 1, 16, 16, 0 in slots 0 .. 4
    before = whole_store(p)
    first, mid, full, last = FIVE_IDS[1], FIVE_IDS[2], FIVE_IDS[3], FIVE_IDS[4]
    assert clear(api, p, [[]])[0] == [0] and whole_store(p) == before       # an empty list
    assert clear(api, p, [[(mid, 3)]])[0] == [1]                            # one entry
    assert clear(api, p, [[(mid, 5), (mid, 6)], [(mid, 7), (mid, 8)]], n=[-2, 11], list_cap=2)[0] == [0, 2]      # d_n below 0 and above list_cap
    # an id not held, a negative id, tag = count - 1 / = count / negative, on the first slot with features and on the last slot (which has none)
    assert clear(api, p, [[(5, 0), (-3, 0), (first, 0), (first, 1), (first, -1), (full, 15), (full, 16), (last, 0)]])[0] == [2]
    assert clear(api, p, [[(FIVE_IDS[0], 0)], [(full, 0), (full, 0), (full, 0)]])[0] == [0, 3]                      # the first slot holds no feature; duplicates
    assert clear(api, p, [[(mid, 9)]], with_count=False)[0] == [1]                                                   # d_n_cleared NULL
    after = whole_store(p)                                                  # WHOLE against the restatement, whose tables the rule changed
    assert after["lm"] != before["lm"] and all(after[k] == before[k] for k in after if k != "lm")
    lm = np.frombuffer(after["lm"], np.int32).reshape(5, F)
    assert lm[1, 0] == -1 and (lm[2, [3, 7, 8, 9]] == -1).all() and lm[3, 15] == -1 and lm[3, 0] == -1
    assert np.count_nonzero(lm != np.frombuffer(before["lm"], np.int32).reshape(5, F)) <= 7
    # pending: the key-frame that is not put yet; its id per item; a tag at feat_cap is not its table's
    new_id = FIVE_IDS[4] + 10
    tab = np.arange(3 * F, dtype=np.int32).reshape(3, F)
    want, tab2 = clear(api, p, [[(new_id, 2), (new_id, F), (mid, 10), (new_id, F - 1)], [(new_id, 1)], [(new_id + 1, 4), (full, 1)]],
                       pending=([new_id, new_id + 5, new_id + 1], tab))
    assert want == [3, 0, 2] and tab2[0, 2] == tab2[0, F - 1] == tab2[2, 4] == -1 and np.count_nonzero(tab2 != tab) == 3
    # the same list as item 0 and as item 2 among other neighbours: the item's pending table and count are the same
    again = clear(api, p, [[(full, 1)], [], [(new_id, 2), (new_id, F), (mid, 10), (new_id, F - 1)]], pending=([7, 8, new_id], tab[[1, 2, 0]]))
    assert again[0][2] == want[0] and _same(again[1][2], tab2[0])
    # a key-frame put after the call holds what its table said
    kps, desc, _ = R.random_keyframes(31, 1, cap, F)
    assert p.put([new_id], kps, desc, [2], None, tab2[:1], [F]) == 0
    got = whole_store(p, extra_ids=[new_id + 99])                           # (and an id that is not held is still refused by detect)
    assert np.frombuffer(got["lm"], np.int32).reshape(7, F)[5].tolist() == tab2[0].tolist()
    # call level: nothing enqueued
    import torch
    d = [_dev(np.zeros((1, 8), np.int64)), _dev(np.zeros((1, 8), np.int32)), _dev(np.zeros(1, np.int32)), _dev(np.zeros(1, np.int64)), _dev(np.zeros((1, F), np.int32))]
    ptr = [x.data_ptr() for x in d]
    torch.cuda.synchronize()

    def code(*a):
        try:
            p.dev.clear_links_batch(*a)
            return 0
        except api.MyslamError as e:
            return e.code

    for k in range(3):
        assert code(*(ptr[:k] + [None] + ptr[k + 1:3]), 8, 1) == api.ERR_INVALID
    assert code(*ptr[:3], 0, 1) == code(*ptr[:3], 8, 0) == code(*ptr[:3], 8, -1) == api.ERR_INVALID
    assert code(*ptr[:3], 8, 1, ptr[3], None) == code(*ptr[:3], 8, 1, None, ptr[4]) == api.ERR_INVALID
    assert code(*ptr[:3], 8, 65536) == api.ERR_CAPACITY
    whole_store(p)                                                          # nothing was enqueued: still the restatement's bytes


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the filter

def test_filter_reads_its_own_items_states_and_the_whole_row(api):
    import torch
    B, P, F = 3, 24, 300                                                    # 300 entries: two passes of the 256-thread block
    arc = api.MapArchive(B + 1, 4, 4, P, 8)
    rng = np.random.default_rng(77)
    n_mp = [10, P, 0]
    states = [rng.integers(0, 3, n).astype(np.uint8) for n in n_mp]
    states[0][[8, 9]] = (0, 2); states[1][P - 1] = 2
    for b in range(B):
        n = n_mp[b]
        arc.load(b, [1], [mi.IDENT], [], [], np.zeros((0, 7)), 10 + np.arange(n), np.zeros((n, 3)), np.full(n, -1, np.int32), states[b])
    arc.load(3, [1], [mi.IDENT], [], [], np.zeros((0, 7)), [10, 11], np.zeros((2, 3)), [-1, -1], [2, 2])
    rows = rng.integers(-1, P + 5, (B, F)).astype(np.int32)
    for b in range(B):                                                      # entries -1, n_mp - 1, n_mp, point_cap + 5, INT_MIN; in both passes of the block
        rows[b, [0, 1, 2, 3, 4]] = (-1, n_mp[b] - 1, n_mp[b], P + 5, INT_MIN)
        rows[b, [F - 5, F - 4, F - 3, F - 2, F - 1]] = (INT_MIN, P + 5, n_mp[b], n_mp[b] - 1, -1)
    d = torch.from_numpy(rows.copy()).cuda(); d_n = torch.full((B + 1,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    arc.filter_landmarks_batch(d.data_ptr(), F, B, d_n.data_ptr())
    torch.cuda.synchronize()
    got, cnt = d.cpu().numpy(), d_n.cpu().numpy()
    for b in range(B):
        want, n = lu.filter_landmarks(rows[b], states[b])
        assert _same(got[b], want) and cnt[b] == n, b
    assert cnt[3] == -9 and cnt[0] > 0 and cnt[1] > 0 and cnt[2] == 0 and _same(got[2], rows[2])
    assert got[0, 1] == -1 and got[0, 2] == 10 and got[1, 1] == -1 and got[1, F - 2] == -1 and (got[:, 3] == P + 5).all() and (got[:, 4] == INT_MIN).all()
    # item b reads item b's states only, wherever the row stands: the rows permuted over the items give other answers, each its own rule's
    d2 = torch.from_numpy(rows[[1, 2, 0]].copy()).cuda()
    torch.cuda.synchronize()
    arc.filter_landmarks_batch(d2.data_ptr(), F, B)                         # d_n_dropped NULL
    torch.cuda.synchronize()
    for b, src in enumerate((1, 2, 0)):
        assert _same(d2.cpu().numpy()[b], lu.filter_landmarks(rows[src], states[b])[0])
    # a batch of one leaves the other rows alone; the same archive content in another slot gives the same bytes
    arc2 = api.MapArchive(2, 4, 4, P, 8)
    arc2.load(1, [1], [mi.IDENT], [], [], np.zeros((0, 7)), 10 + np.arange(10), np.zeros((10, 3)), np.full(10, -1, np.int32), states[0])
    d3 = torch.from_numpy(np.stack([rows[0], rows[0]])).cuda()
    torch.cuda.synchronize()
    arc2.filter_landmarks_batch(d3.data_ptr(), F, 2)
    torch.cuda.synchronize()
    assert _same(d3.cpu().numpy()[1], got[0]) and _same(d3.cpu().numpy()[0], rows[0])          # item 0 of arc2 is an empty map: nothing is erased
    for args, want in (((0, F, 1), api.ERR_INVALID), ((d.data_ptr(), 0, 1), api.ERR_INVALID), ((d.data_ptr(), F, B + 2), api.ERR_CAPACITY)):
        with pytest.raises(api.MyslamError) as e:
            arc.filter_landmarks_batch(*args)
        assert e.value.code == want


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. the tracker

def feature_ids(st, ids):
    """feature -> landmark ID (slot numbers are not comparable between hand-overs)"""
    return np.array([ids["landmark_id"][l] if l >= 0 else -1 for l in st["lm"]], np.int64)


def test_tracker_clears_the_key_frames_own_features(api, pkg, synth):
    import torch
    chain = pkg.chain
    S, L = 8, 8
    rig = InitRig(api, chain, S, good=20, bad=10)
    rich = KC.rich_case(chain, synth)
    for s in (0, 3, 4, 7):
        rig.load(s, rich)                                                   # due for a turn
    idle = KC.make(chain, synth, "no ids", n=30, n_new=0, seed=371)
    idle["st"]["next_frame_id"] = idle["st"]["ref_frame_id"] + 1            # its last frame is its reference frame, but nobody gave it ids
    rig.load(2, idle, why=0, ids=False)
    rig.arm(5, pair(synth, "start", 120, 360))                              # straight from create: takes the init
    rig.load(1, KC.make(chain, synth, "running", n=30, n_new=4, seed=372), why=0)          # running, some frames after its key-frame
    rig.turn()
    out = rig.init(50)
    assert out["report"][5, 0] == 0
    pre = [(rig.state(s), rig.trk.get_ids(s)) for s in range(S)]
    for s in (0, 3, 4, 5, 7):
        assert pre[s][0]["ref_frame_id"] == pre[s][0]["next_frame_id"] - 1 and pre[s][1]["valid"] == 1, s
    assert pre[2][1]["valid"] == 0 and pre[1][0]["ref_frame_id"] != pre[1][0]["next_frame_id"] - 1
    ref = [pre[s][1]["ref_kf_id"] for s in range(S)]
    nf = [len(pre[s][0]["lm"]) for s in range(S)]
    linked = lambda s: np.nonzero(pre[s][0]["lm"] >= 0)[0]
    a0, a5 = linked(0), linked(5)
    lists = [[] for _ in range(S)]
    lists[0] = [(ref[0], int(a0[0])), (ref[0], int(a0[-1])), (ref[0], int(a0[5])), (ref[0], int(a0[5])), (ref[0] + 1, int(a0[7])), (ref[0], nf[0] - 1)]
    lists[1] = [(ref[1], 0), (ref[1], 1)]                                   # stepped since its key-frame
    lists[2] = [(pre[2][1]["ref_kf_id"], 0), (0, 1), (7, 2)]                # ids not valid
    lists[3] = [(ref[3] + 1, 0), (ref[3] - 1, 1), (-1, 2)]                  # wrong key-frame id
    lists[4] = [(ref[4], nf[4]), (ref[4], -1), (ref[4], rig.cap)]           # tag = n_feat, negative, the cap
    lists[5] = [(ref[5], int(a5[0])), (ref[5], int(a5[-1]))]                # after init_batch
    lists[7] = list(lists[0])
    ids = np.full((S, L), -5, np.int64); tags = np.full((S, L), -6, np.int32)
    for s, l in enumerate(lists):
        for j, (k, t) in enumerate(l):
            ids[s, j], tags[s, j] = k, t
    n = np.array([len(l) for l in lists], np.int32)
    n[7] = L + 50                                                           # above list_cap: reads as list_cap (the two spare entries name nothing)
    n[6] = -1
    d = [torch.from_numpy(x).cuda() for x in (ids, tags, n)]
    d_cnt = torch.full((S,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rig.trk.clear_links_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), L, d_cnt.data_ptr())
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    post = [(rig.state(s), rig.trk.get_ids(s)) for s in range(S)]
    for s in range(S):
        st, sid = pre[s]
        trk = dict(ids_valid=sid["valid"], ref_frame_id=st["ref_frame_id"], next_frame_id=st["next_frame_id"], ref_kf_id=sid["ref_kf_id"], lm=st["lm"].copy())
        hits = lu.tracker_clear_links(trk, lists[s] + [(-5, -6)] * L, n=n[s], list_cap=L)
        assert cnt[s] == hits, (s, cnt[s], hits)
        for k in STATE_KEYS:                                                # exactly the named feature slots differ
            assert _same(post[s][0][k], trk["lm"] if k == "lm" else st[k]), (s, k)
        assert all(_same(post[s][1][k], sid[k]) for k in sid), s
        named = sorted({t for k, t in lists[s] if k == sid["ref_kf_id"] and 0 <= t < nf[s]}) if hits else []
        want_ids = feature_ids(st, sid); want_ids[named] = -1
        assert _same(feature_ids(*post[s]), want_ids), s
    assert cnt.tolist() == [5, 0, 0, 0, 0, 2, 0, 5]
    assert (post[0][0]["lm"][[a0[0], a0[-1], a0[5]]] == -1).all() and post[0][0]["lm"][a0[7]] >= 0 and (post[5][0]["lm"][[a5[0], a5[-1]]] == -1).all()
    assert _state_bytes(*post[0]) == _state_bytes(*post[7])                 # the same stream in another slot, among other neighbours
    # one more step: stream 0 against stream 6, which is handed stream 0's state (with the -1s) through set_frame
    rig.trk.set_frame(6, post[0][0], image=post[0][0]["image"])
    rig.trk.set_ids(6, post[0][1]["landmark_id"], post[0][1]["ref_kf_id"], post[0][1]["next_kf_id"], post[0][1]["next_mp_id"])
    rig.marked.add(6)
    nxt = TC.images(synth, 360, 120, 160, (1, 0))[1]
    img = [rich["left"], rig.cases[1]["left"], idle["left"], rich["left"], rich["left"], nxt, rich["left"], rich["left"]]
    d_img = torch.from_numpy(np.stack(img)).cuda()
    d_res = torch.zeros(S * 80, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rig.trk.step_batch(d_img.data_ptr(), 160, 120 * 160, d_res.data_ptr())
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert res[0].tobytes() == res[6].tobytes() and res["n_features"][0] > 10
    assert all(_same(x, y) for x, y in zip(rig.trk.debug_last_step(0), rig.trk.debug_last_step(6)))
    s0, s6 = rig.state(0), rig.state(6)
    assert all(_same(s0[k], s6[k]) for k in STATE_KEYS) and _same(feature_ids(s0, rig.trk.get_ids(0)), feature_ids(s6, rig.trk.get_ids(6)))
    print("features after the step: cleared stream", int(res["n_features"][0]), "its untouched twin", int(res["n_features"][3]))
    assert res["n_features"][0] <= res["n_features"][3]                     # a feature without a landmark is not carried on (src/frontend.cpp:156-170)
    # every stream has stepped once since its key-frame now (or never had one): the same lists touch nothing
    pre2 = [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(S)]
    ids2 = ids.copy()
    for s in range(S):
        ids2[s, :] = rig.trk.get_ids(s)["ref_kf_id"]
    tags2 = np.zeros((S, L), np.int32)
    d2 = [torch.from_numpy(x).cuda() for x in (ids2, tags2, np.full(S, L, np.int32))]
    torch.cuda.synchronize()
    rig.trk.clear_links_batch(d2[0].data_ptr(), d2[1].data_ptr(), d2[2].data_ptr(), L, d_cnt.data_ptr())
    rig.trk.clear_links_batch(d2[0].data_ptr(), d2[1].data_ptr(), d2[2].data_ptr(), L)        # d_n_cleared NULL
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [0] * S and [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(S)] == pre2
    for bad in ((0, d[1].data_ptr(), d[2].data_ptr(), L), (d[0].data_ptr(), 0, d[2].data_ptr(), L), (d[0].data_ptr(), d[1].data_ptr(), 0, L),
                (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0)):
        with pytest.raises(api.MyslamError) as e:
            rig.trk.clear_links_batch(*bad)
        assert e.value.code == api.ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. one recording of clear_links + filter + the tracker call, replayed with other lists and a key-frame put after the recording

def test_one_recording_replayed_with_other_lists_equals_eager_calls(api, pkg, synth):
    import torch
    cap, F, L, P = 37, 16, 8, 40
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def world():
        p = five(api, cap)
        p.dev.set_stream(sp)
        arc = api.MapArchive(2, 4, 4, P, 8, stream=sp)
        for b in range(2):
            arc.load(b, [1], [mi.IDENT], [], [], np.zeros((0, 7)), np.arange(P), np.zeros((P, 3)), np.full(P, -1, np.int32), (np.arange(P) % 3 == b).astype(np.uint8) * 2)
        rig = Rig(api, 2, good=20, bad=10, stream=sp)
        for s in range(2):
            rig.load(s, KC.rich_case(pkg.chain, synth))
        rig.turn()
        return p, arc, rig

    new_id = FIVE_IDS[4] + 3
    kps, desc, _ = R.random_keyframes(41, 1, cap, F)
    new_tab = (np.arange(F, dtype=np.int32) * 2 % P).reshape(1, F)

    def lists_of(p, rig, k):
        ref = [rig.trk.get_ids(s)["ref_kf_id"] for s in range(2)]
        if k == 0:
            return [[(FIVE_IDS[2], 1), (ref[0], 0), (new_id, 3)], [(FIVE_IDS[3], 2), (ref[1], 1)]]
        return [[(new_id, 3), (new_id, 4), (ref[0], 2), (FIVE_IDS[3], 9)], [(ref[1], 3), (new_id, 5), (new_id, F)]]          # new_id: held only after the recording

    def run(recorded):
        p, arc, rig = world()
        bufs = dict(ids=torch.zeros((2, L), dtype=torch.int64, device="cuda"), tags=torch.zeros((2, L), dtype=torch.int32, device="cuda"),
                    n=torch.zeros(2, dtype=torch.int32, device="cuda"), cleared=torch.zeros(2, dtype=torch.int32, device="cuda"),
                    t_cleared=torch.zeros(2, dtype=torch.int32, device="cuda"), dropped=torch.zeros(2, dtype=torch.int32, device="cuda"),
                    q=torch.zeros(2, dtype=torch.int64, device="cuda"), score=torch.ones(2, dtype=torch.float32, device="cuda"),
                    cnt=torch.zeros(2, dtype=torch.int32, device="cuda"))
        o = p.outputs(2)
        ptr = lambda k: bufs[k].data_ptr()

        def body():
            p.dev.clear_links_batch(ptr("ids"), ptr("tags"), ptr("n"), L, 2, None, None, ptr("cleared"))
            rig.trk.clear_links_batch(ptr("ids"), ptr("tags"), ptr("n"), L, ptr("t_cleared"))
            p.launch([bufs["q"], bufs["score"], bufs["cnt"]], o, thr_high=NEG_INF)
            arc.filter_landmarks_batch(o["lm"].data_ptr(), F, 2, ptr("dropped"))

        def feed(k, query):
            ids = np.full((2, L), -1, np.int64); tags = np.full((2, L), -1, np.int32)
            ls = lists_of(p, rig, k)
            for b, l in enumerate(ls):
                for j, (i, t) in enumerate(l):
                    ids[b, j], tags[b, j] = i, t
            with torch.cuda.stream(stream):
                bufs["ids"].copy_(torch.from_numpy(ids)); bufs["tags"].copy_(torch.from_numpy(tags))
                bufs["n"].copy_(torch.from_numpy(np.array([len(l) for l in ls], np.int32)))
                bufs["q"].copy_(torch.from_numpy(np.array(query, np.int64)))
                o["lm"].fill_(-1)
            stream.synchronize()

        torch.cuda.synchronize()
        feed(0, [FIVE_IDS[2], FIVE_IDS[3]])
        g = api.StepGraph.record(sp, [], body) if recorded else None
        if not recorded:
            body()
        else:
            g.launch(sp)
        stream.synchronize()
        snaps = [{k: v.cpu().numpy().copy() for k, v in list(bufs.items())[3:6]} | {"lm": o["lm"].cpu().numpy().copy(), "slot": o["slot"].cpu().numpy().copy()}]
        t = [_dev(kps), _dev(desc), _dev(np.array([2], np.int32)), _dev(new_tab), _dev(np.array([F], np.int32))]
        torch.cuda.synchronize()
        p.dev.put_batch([new_id], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, t[3].data_ptr(), t[4].data_ptr())
        feed(1, [new_id, FIVE_IDS[3]])
        if recorded:
            g.launch(sp)
        else:
            body()
        stream.synchronize()
        snaps.append({k: v.cpu().numpy().copy() for k, v in list(bufs.items())[3:6]} | {"lm": o["lm"].cpu().numpy().copy(), "slot": o["slot"].cpu().numpy().copy()})
        states = [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(2)]
        return snaps, states

    eager, e_states = run(False)
    replay, r_states = run(True)
    for a, b in zip(eager, replay):
        for k in a:
            assert _same(a[k], b[k]), k
    assert e_states == r_states
    assert eager[0]["cleared"].tolist() == [1, 1] and eager[0]["t_cleared"].tolist() == [1, 1]
    assert eager[1]["cleared"].tolist() == [3, 1] and eager[1]["slot"].tolist() == [5, 3]          # the replay sees the key-frame put after the recording
    lm = eager[1]["lm"]
    assert lm[0, 3] == lm[0, 4] == -1 and lm[0, 5] == -1 and eager[1]["dropped"][0] > 0 and lm[1, 9] == -1 and lm[1, 2] == -1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. the histories of tests/test_whole_map_model.py on the device

BATCHES = (T.HISTORIES[:6], T.HISTORIES[6:])
FEAT_CAP, PRIOR_CAP, OUTLIER_CAP = 128, 96, 64
BE_CAPS = (8, 96, 1536)
ARCH_CAPS = (24, 24, 640)
STORE_FEAT = lu.FEAT_CAP
PARKED = mi.Insert(1, mi.IDENT, [(-2, (0.0, 0.0, 0.0), (1.0, 2.0), 7, False)])        # a feature id below -1: refused whatever the table holds
OPT_OUT = ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2", "rounds", "n_out", "status")
LOAD = ("kf_id", "kf_pose", "edge_v0", "edge_v1", "meas", "mp_id", "mp_pos", "mp_first_kf", "mp_state", "snapshot", "mp_gone_kf", "mp_win_mask", "win_kf")


class Item:
    def __init__(self, api, pkg, spec, stream):
        self.spec = spec
        self.m = wm.WholeMap(pkg.chain, spec[1])
        self.gen = wm.history(spec[0], self.m, T.K, spec[2], spec[3], tuple(e for e in spec[4] if e != "capacity"))
        self.window = spec[1]
        self.up, self.ref = lu.Upkeep(), lu.Store(STORE_FEAT)
        self.store = api.LoopKeyFrameStore(spec[2] + 1, 4, STORE_FEAT, stream)
        self.pending = None
        self.log = []                                                       # what the independence test compares


def run_histories(api, pkg, specs):
    """-> the items after every history has run to its end.  specs: a history per item (None = an item nothing happens to)"""
    import torch
    B = len(specs)
    windows = sorted({s[1] for s in specs if s})
    r = InsRun(api, [br.Map() for _ in range(B)], [PARKED] * B, windows[0], 0.2, caps=(BE_CAPS, FEAT_CAP, PRIOR_CAP, OUTLIER_CAP))
    sp = r.stream.cuda_stream
    items = [Item(api, pkg, s, sp) if s else None for s in specs]
    dev = Dev(api, B, ARCH_CAPS, BE_CAPS, r.stream)
    dev.h.attach_solve(*r.h.solve_view())
    full = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
    oo = dict(obs_report=full((B, BE_CAPS[2]), torch.uint8), mp_report=full((B, BE_CAPS[1]), torch.uint8), new_outlier=full((B, BE_CAPS[1]), torch.int32),
              n_new=full((B,), torch.int32), obs_chi2=full((B, BE_CAPS[2]), torch.float64), rounds=full((B,), torch.int32), n_out=full((B,), torch.int32),
              status=full((B,), torch.int32))
    c_kf, c_tag, c_n = culled_tensors(r.h, B, BE_CAPS[2])
    d_feat, d_nf = full((B, STORE_FEAT), torch.int64, -1), full((B,), torch.int32)
    d_tab, d_pid = full((B, STORE_FEAT), torch.int32, -1), full((B,), torch.int64, -1)
    d_ncl, d_ndrop = full((B,), torch.int32), full((B,), torch.int32)
    d_kps, d_desc, d_zero = full((1, 4, 28), torch.uint8), full((1, 4, 32), torch.uint8), full((1,), torch.int32)
    r.stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()

    def tables():
        r.stream.synchronize()
        return {k: v.cpu().numpy() for k, v in r.d.items()}

    while True:
        evs, corrected = [], []
        for b, it in enumerate(items):
            ev = next(it.gen, None) if it else None
            while ev is not None and ev.kind == "correct":
                it.m.correct(ev.rigid, ev.moves)
                if b not in corrected:
                    corrected.append(b)
                ev = next(it.gen, None)
            evs.append(ev)
        if all(ev is None for ev in evs):
            break
        if corrected:                                                       # the archive is overwritten with the moved values, write_backend carries them on
            sel = np.zeros(B, np.uint8); sel[corrected] = 1
            r.stream.synchronize()
            for b in corrected:
                it, arch = items[b], dev.h.get(b)
                for row, kid in enumerate(arch["kf_id"]):
                    arch["kf_pose"][row] = it.m.all_kfs[int(kid)].pose
                for s, mid in enumerate(arch["mp_id"]):
                    if int(mid) in it.m.all_mps:
                        arch["mp_pos"][s] = it.m.all_mps[int(mid)].pos
                dev.h.load(b, *[arch[k] for k in LOAD])
            d_sel = torch.from_numpy(sel).cuda()
            torch.cuda.synchronize()
            dev.h.write_backend_batch(p(r.d["kf_id"]), p(r.d["kf_pose"]), p(r.d["n_kf"]), BE_CAPS[0], p(r.d["mp_id"]), p(r.d["mp_pos"]), p(r.d["n_mp"]), BE_CAPS[1],
                                      p(d_sel), B)
            r.stream.synchronize()
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
            dev.update(0, r.d, r.o["status"], r.di["outlier_mp_id"], r.di["n_outlier"], OUTLIER_CAP)
            r.stream.synchronize()
            st, ast = r.o["status"].cpu().numpy(), dev.status.cpu().numpy()
            for b, (it, ev) in enumerate(zip(items, evs)):
                if ev is None or it.window != W:
                    assert st[b] == mi.INVALID
                elif ev.kind == "refused":
                    assert st[b] == mi.INVALID and it.m.insert_keyframe(ev.ins)["status"] == wm.INVALID
                else:
                    assert ev.kind == "insert" and st[b] == mi.OK and ast[b] == 0, (it.spec, st[b], ast[b])
                    assert it.m.insert_keyframe(ev.ins)["status"] == wm.OK
                    it.pending = ev.ins
                    it.up.feats[ev.ins.kf_id] = list(ev.ins.feats); it.up.order.append(ev.ins.kf_id)
        # ---- the optimise, with the device's own solve
        opts = [next(it.gen, None) if ev is not None else None for it, ev in zip(items, evs)]
        assert all(o is None or o.kind == "optimize" for o in opts)
        host = tables()
        r.h.optimize_batch(*[p(r.d[k]) for k in TABLE_ARGS], B, T.K, *[p(oo[k]) for k in OPT_OUT])
        dev.update(1, r.d, oo["status"], report=oo["mp_report"])
        after = tables()
        rep = {k: v.cpu().numpy() for k, v in oo.items()}
        ck, ct, cn = c_kf.cpu().numpy(), c_tag.cpu().numpy(), c_n.cpu().numpy()
        entries = [[] for _ in range(B)]
        for b, (it, ev) in enumerate(zip(items, opts)):
            if ev is None:
                assert cn[b] == 0
                continue
            n_mp, n_obs = int(host["n_mp"][b]), int(host["n_obs"][b])
            t_in = {k: host[k][b] for k in ("kf_id", "mp_id", "obs_kf", "obs_tag")} | {"obs_mp": host["obs_mp"][b, :n_obs]}
            flat = r.h.debug_flat(b)
            poses = lambda b=b: {int(k): after["kf_pose"][b, i] for i, k in enumerate(after["kf_id"][b, :int(after["n_kf"][b])])}

            def points(b=b, t_in=t_in, flat=flat):
                x = r.h.debug_solved(b)[1]
                return {int(t_in["mp_id"][row]): x[j] for j, row in enumerate(flat["pt_src"])}

            before_all = set(it.m.all_mps)
            rm = it.m.optimize(ev.flags, poses, points)
            assert rep["status"][b] == rm["status"], (it.spec, rep["status"][b])
            if rm["status"] == br.DONE:
                assert np.array_equal(rep["obs_report"][b, :n_obs], rm["obs_report"]) and np.array_equal(rep["mp_report"][b, :n_mp], rm["mp_report"]), it.spec
                it.up.note_erased(it.m, before_all, rm)
                entries[b] = lu.culled_list(t_in, rm["obs_report"])         # the model's removals, by the tables the call read
            assert cn[b] == len(entries[b]) and list(zip(ck[b, :cn[b]].tolist(), ct[b, :cn[b]].tolist())) == entries[b], (it.spec, cn[b])
            it.up.count_list(entries[b], it.pending.kf_id if it.pending else None, it.ref.ids)
        # ---- link upkeep: the turn's feature-slot table, the culled lists straight from the back end's buffers into every item's store, then the put
        feat = np.full((B, STORE_FEAT), -1, np.int64); nf = np.zeros(B, np.int32); pid = np.full(B, -1, np.int64)
        for b, it in enumerate(items):
            if it and it.pending:
                feat[b], nf[b] = lu.feat_ids_by_tag(it.pending.feats, STORE_FEAT)
                pid[b] = it.pending.kf_id
        with torch.cuda.stream(r.stream):
            d_feat.copy_(torch.from_numpy(feat)); d_nf.copy_(torch.from_numpy(nf)); d_pid.copy_(torch.from_numpy(pid)); d_tab.fill_(-1); d_ncl.fill_(-7)
        dev.h.feature_slots_batch(p(d_feat), p(d_nf), STORE_FEAT, B, p(d_tab))
        r.stream.synchronize()
        tab0 = d_tab.cpu().numpy()
        for b, it in enumerate(items):
            if it:
                it.store.clear_links_batch(p(c_kf) + b * BE_CAPS[2] * 8, p(c_tag) + b * BE_CAPS[2] * 4, p(c_n) + b * 4, BE_CAPS[2], 1,
                                           p(d_pid) + b * 8, p(d_tab) + b * STORE_FEAT * 4, p(d_ncl) + b * 4)
        r.stream.synchronize()
        tab1, ncl = d_tab.cpu().numpy(), d_ncl.cpu().numpy()
        for b, it in enumerate(items):
            if not it:
                assert ncl[b] == -7 and _same(tab1[b], tab0[b])
                continue
            want = tab0[b].copy()
            hits = it.ref.clear_links(entries[b], pending_id=int(pid[b]), pending=want)
            assert ncl[b] == hits and _same(tab1[b], want), (it.spec, ncl[b], hits)
            it.log.append((ncl[b], tab1[b].tobytes()))
            if it.pending:
                arch = dev.h.get(b)
                filt = lu.filter_landmarks(tab1[b], arch["mp_state"])[0]
                assert _same(filt, lu.model_links(it.m, arch["mp_id"], it.pending.kf_id, it.pending.feats, STORE_FEAT)), (it.spec, it.pending.kf_id)
                if lu.stored(len(it.up.order) - 1):
                    it.ref.put(it.pending.kf_id, tab1[b], nf[b])
                    it.store.put_batch([it.pending.kf_id], p(d_kps), p(d_desc), p(d_zero), 0, p(d_tab) + b * STORE_FEAT * 4, p(d_nf) + b * 4)
                it.pending = None
        r.stream.synchronize()
        # ---- every stored key-frame of every item: gathered, filtered by the archive, against the model
        nq = [len(it.ref.ids) if it else 0 for it in items]
        if max(nq):
            gath = []
            for b, it in enumerate(items):
                g = full((max(nq[b], 1), STORE_FEAT), torch.int32, -1)
                if nq[b]:
                    q = [torch.tensor(it.ref.ids, dtype=torch.int64, device="cuda"), full((nq[b],), torch.float32, 1), full((nq[b],), torch.int32)]
                    o = [full((nq[b], 4, 32), torch.uint8), full((nq[b],), torch.int32), full((nq[b], 4, 28), torch.uint8), full((nq[b],), torch.int32),
                         full((nq[b],), torch.int32, -5)]
                    torch.cuda.synchronize()
                    it.store.detect_batch(p(q[0]), p(q[1]), p(q[2]), nq[b], p(o[0]), p(o[1]), p(o[2]), p(g), p(o[3]), p(o[4]), thr_high=NEG_INF)
                    r.stream.synchronize()
                    assert o[4].cpu().numpy().tolist() == [0] * nq[b] and o[3].cpu().numpy().tolist() == list(range(nq[b]))
                gath.append(g)
            rows = [dict() for _ in range(B)]; filtered = [dict() for _ in range(B)]
            for k in range(max(nq)):
                tq = torch.stack([gath[b][k] if k < nq[b] else gath[b][0] * 0 - 1 for b in range(B)]).contiguous()
                raw = tq.cpu().numpy()
                torch.cuda.synchronize()
                dev.h.filter_landmarks_batch(p(tq), STORE_FEAT, B, p(d_ndrop))
                r.stream.synchronize()
                out, nd = tq.cpu().numpy(), d_ndrop.cpu().numpy()
                for b, it in enumerate(items):
                    if k < nq[b]:
                        kf_id = it.ref.ids[k]
                        assert _same(raw[b], it.ref.gather(kf_id)), (it.spec, kf_id)
                        rows[b][kf_id], filtered[b][kf_id] = raw[b], out[b]
                        assert nd[b] == int((raw[b] != out[b]).sum())
                        it.log.append((nd[b], out[b].tobytes()))
            for b, it in enumerate(items):
                if it and nq[b]:
                    it.up.check_rows(it.m, dev.h.get(b)["mp_id"], rows[b], filtered[b])
    for it in items:
        if it:
            assert len(it.up.order) == it.spec[2]
    return items


@pytest.mark.parametrize("n", range(len(BATCHES)))
def test_histories_on_the_device(api, pkg, n):
    items = run_histories(api, pkg, list(BATCHES[n]))
    seen = {k: sum(it.up.seen[k] for it in items) for k in lu.CASES}
    print("batch %d:" % n, seen)
    assert all(v > 0 for v in seen.values()), seen


def test_history_items_do_not_depend_on_slot_or_neighbours(api, pkg):
    two = [BATCHES[0][1], BATCHES[0][3]]
    first = run_histories(api, pkg, [two[0], two[1], None])
    second = run_histories(api, pkg, [None, two[1], two[0]])
    assert first[0].log == second[2].log and first[1].log == second[1].log and first[0].log != first[1].log
