"""myslam_backend_insert_keyframe_batch (csrc/backend.hip, k_backend_insert): Map::InsertKeyFrame (src/map.cpp:17-48, :78-140) for a batch of active maps
in device tables.  Every in/out table and every report is compared WHOLE (sentinels beyond the counts included) and byte for byte against
tests/map_insert_ref.py's literal walk fed the device's own distances; the distances are compared on their own with the oracle's |log| to 1e-12, and the
walk fed the ORACLE's distances must choose the same victim.  Then the call's contract: statuses, untouched bytes, slot independence, chaining with
myslam_backend_optimize_batch, graph recording."""
import math

import numpy as np
import pytest

import backend_ref as br
import map_insert_ref as mi

pytestmark = pytest.mark.gpu

IN_OUT = br.TABLES + ("n_kf", "n_mp", "n_obs")
OUT_FILL = dict(feat_row=-71, mp_new_row=-72, removed_kf_id=-73, removed_kf_row=-74, dis=-7.25, status=-75)
TABLE_ARGS = ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def caps_for(maps, inss, slack=(0, 3, 7)):
    """caps that hold every item before and after: (kf_cap, mp_cap, obs_cap), feat_cap, prior_cap, outlier_cap"""
    t = [br.pack(m) for m in maps]
    feat_cap = max(len(i.feats) for i in inss) + 2
    prior_cap = max(len(i.priors) for i in inss) + 1
    outlier_cap = max(len(i.outlier_ids) for i in inss) + 1
    kf = max(len(x["kf_id"]) for x in t) + 1 + slack[0]
    mp = max(len(x["mp_id"]) + len(set(f[0] for f in i.feats)) for x, i in zip(t, inss)) + slack[1]
    obs = max(len(x["obs_mp"]) + len(i.feats) + len(i.priors) for x, i in zip(t, inss)) + slack[2]
    return (kf, mp, max(obs, feat_cap, prior_cap)), feat_cap, prior_cap, outlier_cap


class Run:
    """the tables and the new key-frames of one batch on the device, one call, everything read back"""

    def __init__(self, api, maps, inss, window, th, caps=None, handle=None, prior=True, outlier=True):
        import torch
        self.torch, self.api, self.window, self.th, self.prior, self.outlier = torch, api, window, th, prior, outlier
        self.caps, self.feat_cap, self.prior_cap, self.outlier_cap = caps or caps_for(maps, inss)
        self.B = len(maps)
        self.host = br.pack_batch(maps, *self.caps)
        self.inp = mi.pack_inputs(inss, self.feat_cap, self.prior_cap, self.outlier_cap)
        self.alloc()
        self.stream = torch.cuda.Stream()
        self.h = handle or api.Backend(self.B, *self.caps)
        self.h.set_stream(self.stream.cuda_stream)

    def alloc(self):
        torch, B = self.torch, self.B
        kf_cap, mp_cap, obs_cap = self.caps
        self.d = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.host.items()}
        self.di = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.inp.items()}
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        self.o = dict(feat_row=full((B, self.feat_cap), OUT_FILL["feat_row"], torch.int32), mp_new_row=full((B, mp_cap), OUT_FILL["mp_new_row"], torch.int32),
                      removed_kf_id=full((B,), OUT_FILL["removed_kf_id"], torch.int64), removed_kf_row=full((B,), OUT_FILL["removed_kf_row"], torch.int32),
                      dis=full((B, kf_cap), OUT_FILL["dis"], torch.float64), status=full((B,), OUT_FILL["status"], torch.int32))

    def restore(self):
        with self.torch.cuda.stream(self.stream):
            for k in IN_OUT:
                self.d[k].copy_(self.torch.from_numpy(self.host[k]))
            for k, v in self.inp.items():
                self.di[k].copy_(self.torch.from_numpy(v))
            for k, v in self.o.items():
                v.fill_(OUT_FILL[k])

    def enqueue(self, batch=None, window=None, **over):
        d, di, o = self.d, self.di, self.o
        p = lambda t: t.data_ptr()
        prior = [p(di[k]) for k in ("prior_mp_id", "prior_kf_id", "prior_uv", "prior_tag", "prior_flags", "n_prior")] if self.prior else [None] * 6
        outl = [p(di["outlier_mp_id"]), p(di["n_outlier"])] if self.outlier else [None, None]
        args = [p(d[k]) for k in TABLE_ARGS] + [p(di[k]) for k in ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags",
                                                                  "n_feat")]
        args += [self.feat_cap] + prior + [self.prior_cap] + outl + [self.outlier_cap, self.B if batch is None else batch,
                                                                      self.window if window is None else window, self.th]
        args += [p(o[k]) for k in ("feat_row", "mp_new_row", "removed_kf_id", "removed_kf_row", "dis", "status")]
        for i, v in over.items():
            args[int(i[1:])] = v
        self.h.insert_keyframe_batch(*args)

    def results(self):
        self.stream.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.d.items()}
        out.update({k: v.cpu().numpy() for k, v in self.o.items()})
        return out

    def __call__(self, **kw):
        self.stream.wait_stream(self.torch.cuda.current_stream())
        self.enqueue(**kw)
        return self.results()


def expected_item(r, inp, b, m_after, rep, n_feat):
    """item b's tables and reports as they must be, WHOLE: the walk's state over the input's bytes, the reports over their sentinels"""
    kf_cap, mp_cap, obs_cap = r.caps
    want = {k: inp[k][b].copy() for k in IN_OUT}
    fr = np.full(r.feat_cap, OUT_FILL["feat_row"], np.int32); mr = np.full(mp_cap, OUT_FILL["mp_new_row"], np.int32)
    cf, cm = min(max(n_feat, 0), r.feat_cap), min(max(int(inp["n_mp"][b]), 0), mp_cap)
    if rep["status"] == mi.OK:
        t = br.pack(m_after)
        for k in br.TABLES:
            want[k][:len(t[k])] = t[k]
        want["n_kf"], want["n_mp"], want["n_obs"] = np.int32(len(t["kf_id"])), np.int32(len(t["mp_id"])), np.int32(len(t["obs_mp"]))
        fr[:cf] = rep["feat_row"]; mr[:cm] = rep["mp_new_row"]
    else:
        fr[:cf] = -1; mr[:cm] = -1
    dis = np.full(kf_cap, -1.0)
    if rep["status"] == mi.OK:
        dis[:len(rep["dis"])] = rep["dis"]
    want.update(feat_row=fr, mp_new_row=mr, removed_kf_id=np.int64(rep["removed_kf_id"]), removed_kf_row=np.int32(rep["removed_kf_row"]), dis=dis,
                status=np.int32(rep["status"]))
    return want


def check_item(r, inp, out, b, m_before, ins, window=None, force_status=None, dist=None):
    """walk item b with the device's own distances (`dist`: where the device refuses after computing them, and reports none); compare everything"""
    d = out["dis"][b]
    m = m_before.clone()
    if force_status is None:
        rep = mi.insert_walk(m, ins, r.window if window is None else window, r.th, dist or (lambda pk, pn, row: d[row]), caps=r.caps)
    else:
        rep = dict(status=force_status, removed_kf_id=-1, removed_kf_row=-1)
    want = expected_item(r, inp, b, m, rep, int(r.inp["n_feat"][b]))
    for k, v in want.items():
        got = out[k][b]
        if k == "dis":
            assert _same(np.nan_to_num(got, nan=12345.0), np.nan_to_num(np.asarray(v), nan=12345.0)), (b, k, got, v)
        else:
            assert _same(got, np.asarray(v)), (b, k)
    return m, rep


def oracle_dis(oracle, pk, pn):
    d = oracle.se3_log(oracle.se3_compose(pk, pn, invert_b=True))
    s = 0.0
    for k in range(6):
        s += d[k] * d[k]
    return math.sqrt(s)


def check_distances(oracle, out, b, m_before, ins, rep):
    """d_dis against the oracle's |log(T_kf T_new^-1)| to 1e-12 x max(1, d) (the bar of tests/test_gpu_loop_correct.py for SE3 products)"""
    if rep["status"] != mi.OK or rep["removed_kf_row"] < 0:
        return
    for row, kid in enumerate(sorted(m_before.kfs)):
        want, got = oracle_dis(oracle, m_before.kfs[kid], ins.kf_pose), out["dis"][b, row]
        assert (math.isnan(want) and math.isnan(got)) or abs(got - want) <= 1e-12 * max(1.0, want), (b, row, got, want)


# ---------------------------------------------------------------------------------------------------------------------------------------------
CASES = mi.cases()


@pytest.fixture(scope="module")
def cases():
    return CASES


@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_case_is_the_walk(api, oracle, name):
    case = CASES[name]
    r = Run(api, [case["m"]], [case["ins"]], case["window"], case["th"])
    out = r()
    refused = case.get("status", mi.OK) != mi.OK
    m, rep = check_item(r, r.host, out, 0, case["m"], case["ins"], dist=(lambda pk, pn, row: oracle_dis(oracle, pk, pn)) if refused else None)
    assert rep["status"] == case.get("status", mi.OK) == out["status"][0]
    check_distances(oracle, out, 0, case["m"], case["ins"], rep)
    if "victim_row" in case:
        assert out["removed_kf_row"][0] == case["victim_row"]
        m2 = case["m"].clone()                                              # the oracle's distances choose the same victim
        rep2 = mi.insert_walk(m2, case["ins"], case["window"], case["th"], lambda pk, pn, row: oracle_dis(oracle, pk, pn))
        assert rep2["removed_kf_row"] == out["removed_kf_row"][0] and rep2["removed_kf_id"] == out["removed_kf_id"][0]
    if "exact" in case:
        assert out["dis"][0, :len(case["exact"])].tolist() == case["exact"]


def test_optional_inputs_absent(api, cases):
    case = cases["interleaved_removal"]
    assert not case["ins"].priors and not case["ins"].outlier_ids
    ref = Run(api, [case["m"]], [case["ins"]], case["window"], case["th"])()
    for prior, outlier in ((False, True), (True, False), (False, False)):
        r = Run(api, [case["m"]], [case["ins"]], case["window"], case["th"], prior=prior, outlier=outlier)
        out = r()
        for k in out:
            assert _same(out[k], ref[k]), (prior, outlier, k)
        check_item(r, r.host, out, 0, case["m"], case["ins"])
    # a prior table without its count is no prior table: the rows of 104 are not read
    case = cases["prior_rows_removal"]
    r = Run(api, [case["m"]], [case["ins"]], case["window"], case["th"], prior=False)
    out = r()
    bare = mi.Insert(case["ins"].kf_id, case["ins"].kf_pose, case["ins"].feats)
    check_item(r, r.host, out, 0, case["m"], bare)


def _trio(cases):
    names = ("interleaved_removal", "prior_rows_removal", "victim_middle")
    return [cases[n]["m"] for n in names], [cases[n]["ins"] for n in names]


def _bad_cases(r):
    """name -> (dict to mutate, key, index within item 1, value)"""
    t, i = r.host, r.inp
    n_obs = int(t["n_obs"][1])
    mid = n_obs // 2
    while t["obs_mp"][1, mid] == t["obs_mp"][1, mid - 1]:
        mid += 1
    act = int(np.nonzero(t["obs_flags"][1, :n_obs] & br.ACTIVE)[0][2])
    return {
        "n_kf negative": (t, "n_kf", (), -1), "n_mp beyond its cap": (t, "n_mp", (), 10 ** 6), "n_obs negative": (t, "n_obs", (), -2),
        "n_obs beyond its cap": (t, "n_obs", (), r.caps[2] + 1), "n_feat negative": (i, "n_feat", (), -1), "n_feat beyond its cap": (i, "n_feat", (), r.feat_cap + 1),
        "n_prior negative": (i, "n_prior", (), -1), "n_prior beyond its cap": (i, "n_prior", (), r.prior_cap + 1),
        "n_outlier negative": (i, "n_outlier", (), -1), "n_outlier beyond its cap": (i, "n_outlier", (), r.outlier_cap + 1),
        "kf ids equal": (t, "kf_id", 1, int(t["kf_id"][1, 0])), "mp ids descending": (t, "mp_id", 3, int(t["mp_id"][1, 2]) - 1),
        "obs_mp decreasing": (t, "obs_mp", mid, int(t["obs_mp"][1, mid - 1]) - 1), "obs_mp >= n_mp": (t, "obs_mp", n_obs - 1, int(t["n_mp"][1])),
        "obs_kf >= n_kf": (t, "obs_kf", 1, int(t["n_kf"][1])), "ACTIVE row of a key-frame that left": (t, "obs_kf", act, -1),
        "new id not above the last": (i, "new_kf_id", (), int(t["kf_id"][1, int(t["n_kf"][1]) - 1])),
        "feature id below -1": (i, "feat_mp_id", 2, -2), "prior ids decreasing": (i, "prior_mp_id", 3, 102),
        "prior flag ACTIVE": (i, "prior_flags", 1, br.ACTIVE), "prior flag with another bit": (i, "prior_flags", 0, 4),
        "feature flag ACTIVE": (i, "feat_flags", 0, br.ACTIVE), "feature flag with another bit": (i, "feat_flags", 1, 0x80),
    }


def test_refused_items_keep_every_byte_and_the_neighbours_their_results(api, cases):
    maps, inss = _trio(cases)
    window, th = 3, 0.2
    alone = []
    for m, i in zip(maps, inss):
        r = Run(api, [m], [i], window, th, caps=caps_for(maps, inss))
        alone.append(r())
    proto = Run(api, maps, inss, window, th)
    h = proto.h
    good = proto()
    for b in range(3):
        for k in good:
            assert _same(good[k][b], alone[b][k][0]), (b, k)
        check_item(proto, proto.host, good, b, maps[b], inss[b])
    for name, (_, key, idx, val) in _bad_cases(proto).items():
        r = Run(api, maps, inss, window, th, caps=(proto.caps, proto.feat_cap, proto.prior_cap, proto.outlier_cap), handle=h)
        which = r.host if key in r.host else r.inp
        which[key][(1,) + tuple(np.atleast_1d(idx))] = val
        r.alloc()
        out = r()
        assert out["status"].tolist() == [0, mi.INVALID, 0], name
        check_item(r, r.host, out, 1, maps[1], inss[1], force_status=mi.INVALID)
        for b in (0, 2):
            for k in out:
                assert _same(out[k][b], good[k][b]), (name, b, k)
    # window < 1 refuses every item
    r = Run(api, maps, inss, 0, th, caps=(proto.caps, proto.feat_cap, proto.prior_cap, proto.outlier_cap), handle=h)
    out = r()
    for b in range(3):
        check_item(r, r.host, out, b, maps[b], inss[b], force_status=mi.INVALID)


def test_capacity_per_item(api, cases):
    """the counts BEFORE the removal against the caps: one beyond is refused, exactly at the cap passes"""
    maps, inss = _trio(cases)
    base, feat_cap, prior_cap, outlier_cap = caps_for(maps, inss, slack=(0, 0, 0))
    need = []
    for m, i in zip(maps, inss):
        t = br.pack(m)
        new = set(f[0] for f in i.feats if f[0] >= 0 and f[0] not in m.mps)
        used = [p for p in i.priors if p[0] in new]
        need.append((len(t["kf_id"]) + 1, len(t["mp_id"]) + len(new), len(t["obs_mp"]) + sum(f[0] >= 0 for f in i.feats) + len(used)))
    for axis in range(3):
        worst = max(range(3), key=lambda b: need[b][axis])
        for short in (0, 1):
            caps = [max(n[a] for n in need) + 4 for a in range(3)]
            caps[axis] = need[worst][axis] - short
            assert caps[2] >= max(feat_cap, prior_cap)
            r = Run(api, maps, inss, 3, 0.2, caps=(tuple(caps), feat_cap, prior_cap, outlier_cap))
            out = r()
            want = [(mi.CAPACITY if short and need[b][axis] == need[worst][axis] else 0) for b in range(3)]
            assert out["status"].tolist() == want and mi.CAPACITY in want + [mi.CAPACITY] * (1 - short) and 0 in want, (axis, short)
            for b in range(3):
                m, rep = check_item(r, r.host, out, b, maps[b], inss[b])
                assert rep["status"] == out["status"][b]


def test_call_level(api, cases):
    maps, inss = _trio(cases)
    r = Run(api, maps, inss, 3, 0.2)
    full = r()
    r.restore()
    r.stream.synchronize()

    def refused(code, **kw):
        with pytest.raises(api.MyslamError) as e:
            r.enqueue(**kw)
        assert e.value.code == code, kw
        out = r.results()
        for k in IN_OUT:
            assert _same(out[k], r.host[k]), (kw, k)                       # nothing was enqueued
        assert (out["status"] == OUT_FILL["status"]).all()

    refused(api.ERR_CAPACITY, batch=r.B + 1)
    refused(api.ERR_INVALID, batch=-1)
    refused(api.ERR_INVALID, a0=None)                                       # d_kf_id
    refused(api.ERR_INVALID, a15=None)                                      # d_feat_mp_id
    refused(api.ERR_INVALID, a40=None)                                      # d_status
    refused(api.ERR_INVALID, a23=None)                                      # d_prior_kf_id with a prior count
    refused(api.ERR_INVALID, a29=None)                                      # d_outlier_mp_id with an outlier count
    refused(api.ERR_INVALID, a21=-1)                                        # feat_cap
    refused(api.ERR_CAPACITY, a21=r.caps[2] + 1)                            # feat_cap beyond obs_cap
    refused(api.ERR_CAPACITY, a28=r.caps[2] + 1)                            # prior_cap beyond obs_cap
    r.enqueue(batch=0)                                                      # an empty batch is no error and no work
    out = r.results()
    assert all(_same(out[k], r.host[k]) for k in IN_OUT) and (out["status"] == OUT_FILL["status"]).all()
    r.enqueue(batch=2)                                                      # a batch below the handle's: the last item is not touched
    out = r.results()
    for k in out:
        assert _same(out[k][:2], full[k][:2]), k
        assert _same(out[k][2], (r.host[k] if k in r.host else np.full_like(full[k], OUT_FILL[k]))[2]), k
    assert r.h.insert_launches_per_call() == 1 and r.h.launches_per_call() == 3


def test_slot_independence(api, cases):
    names = ("interleaved_removal", "prior_rows_removal", "victim_middle", "outlier_ids_removal", "two_and_three_on_one_id_removal")
    maps, inss = [cases[n]["m"] for n in names], [cases[n]["ins"] for n in names]
    caps = caps_for(maps, inss)
    batch = Run(api, maps, inss, 3, 0.2, caps=caps)()
    rev = Run(api, maps[::-1], inss[::-1], 3, 0.2, caps=caps)()
    for b in range(5):
        alone = Run(api, [maps[b]], [inss[b]], 3, 0.2, caps=caps)()
        for k in batch:
            assert _same(batch[k][b], alone[k][0]), (b, k)
            assert _same(batch[k][b], rev[k][4 - b]), (b, k)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# chaining with myslam_backend_optimize_batch

OPT_FILL = dict(obs_report=0xCC, mp_report=0xCB, new_outlier=-55, n_new=-56, obs_chi2=-3.25, rounds=-57, n_out=-58, status=-59)


def next_keyframe(chain, m, K, step, rng):
    """a key-frame that follows the map's last: most features on active map points at their projections, a few new ids (above, and between where an
    id is free), a few features without a map point; every third step two ids from the outlier list"""
    kf_ids = sorted(m.kfs)
    pose = m.kfs[kf_ids[-1]].copy()
    pose[4:] += rng.uniform(-0.05, 0.05, 3) + (0.0, 0.0, -0.1)
    T = chain.T_of(pose)
    fx, fy, cx, cy = K
    ids = sorted(m.mps)
    feats = []
    for n, mid in enumerate(rng.permutation(ids)[:45].tolist()):
        pc = T[:3, :3] @ m.mps[mid].pos + T[:3, 3]
        uv = (fx * pc[0] / pc[2] + cx + rng.normal(0, 0.3), fy * pc[1] / pc[2] + cy + rng.normal(0, 0.3))
        feats.append((mid, tuple(m.mps[mid].pos), tuple(np.float32(uv)), 10 ** 6 * (step + 1) + n, False))
        if n % 9 == 0:
            feats.append((-1, (0.0, 0.0, 0.0), (1.0, 2.0), 10 ** 6 * (step + 1) + 500 + n, False))
    free = [i for i in range(ids[0], ids[-1]) if i not in m.mps][:2]
    Ti = np.linalg.inv(T)
    for n, mid in enumerate(free + [ids[-1] + 2, ids[-1] + 3, ids[-1] + 7]):
        pc = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(8, 20)])
        pw = Ti[:3, :3] @ pc + Ti[:3, 3]
        feats.append((mid, tuple(pw), (np.float32(fx * pc[0] / pc[2] + cx), np.float32(fy * pc[1] / pc[2] + cy)), 10 ** 6 * (step + 1) + 900 + n, False))
    outl = rng.permutation(ids)[:2].tolist() if step % 3 == 2 else []
    return mi.Insert(kf_ids[-1] + 1 + step % 2, pose, feats, outlier_ids=outl)


def test_chaining_insert_and_optimise(api, pkg, synth):
    """12 key-frames through insert -> optimise -> insert ... on 3 maps: the tables stay on the device (they are only read back, never written by the
    host); after every call they are the walks', fed the device's distances and the device's solve"""
    import torch
    made = [br.make_map(synth, s, n_kf=6, n_mp=60) for s in (0x300, 0x301, 0x302)]
    cur, K = [x[0].clone() for x in made], made[0][1]
    caps, feat_cap, window = (8, 160, 1600), 64, 7
    rng = np.random.default_rng(0xC4A1)
    first = [next_keyframe(pkg.chain, m, K, 0, rng) for m in cur]
    r = Run(api, cur, first, window, 0.2, caps=(caps, feat_cap, 2, 4))
    B = 3
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    oo = dict(obs_report=full((B, caps[2]), 0, torch.uint8), mp_report=full((B, caps[1]), 0, torch.uint8), new_outlier=full((B, caps[1]), 0, torch.int32),
              n_new=full((B,), 0, torch.int32), obs_chi2=full((B, caps[2]), 0, torch.float64), rounds=full((B,), 0, torch.int32),
              n_out=full((B,), 0, torch.int32), status=full((B,), 0, torch.int32))
    r.stream.wait_stream(torch.cuda.current_stream())
    removed = left = 0
    for step in range(12):
        inss = first if step == 0 else [next_keyframe(pkg.chain, m, K, step, rng) for m in cur]
        r.inp = mi.pack_inputs(inss, feat_cap, 2, 4)
        with torch.cuda.stream(r.stream):
            for k, v in r.inp.items():
                r.di[k].copy_(torch.from_numpy(v))
            for k, v in r.o.items():
                v.fill_(OUT_FILL[k])
        r.stream.synchronize()
        inp = {k: v.cpu().numpy() for k, v in r.d.items()}
        r.enqueue()
        out = r.results()
        for b in range(B):
            m, rep = check_item(r, inp, out, b, cur[b], inss[b])
            assert rep["status"] == mi.OK
            cur[b] = m
            removed += int(rep["removed_kf_row"] >= 0); left += int((rep["mp_new_row"] < 0).sum())
        with torch.cuda.stream(r.stream):
            for k, v in oo.items():
                v.fill_(OPT_FILL[k])
        r.h.optimize_batch(*[r.d[k].data_ptr() for k in TABLE_ARGS], B, K,
                           *[oo[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2", "rounds", "n_out", "status")])
        r.stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in r.d.items()}
        st = oo["status"].cpu().numpy()
        for b in range(B):
            def solve(poses, pts, ep, el, eo, fixed, b=b):
                return r.h.debug_solved(b)
            rep = br.walk(cur[b], solve)
            assert st[b] == rep["status"] == br.DONE, (step, b)
            want = br.pack(cur[b])
            for k in br.TABLES:
                assert _same(got[k][b, :len(want[k])], want[k]), (step, b, k)
            assert (got["n_kf"][b], got["n_mp"][b], got["n_obs"][b]) == (len(want["kf_id"]), len(want["mp_id"]), len(want["obs_mp"]))
    assert removed >= 30 and left > 0


def test_recorded_step_replays_on_other_tables(api, cases):
    """insert + optimise recorded once, replayed on tables with other contents and other counts"""
    import torch
    a = ("interleaved_removal", "prior_rows_removal", "victim_middle")
    b = ("victim_last", "two_and_three_on_one_id_removal", "outlier_ids_removal")
    ma, ia = [cases[n]["m"] for n in a], [cases[n]["ins"] for n in a]
    mb, ib = [cases[n]["m"] for n in b], [cases[n]["ins"] for n in b]
    caps = caps_for(ma + mb, ia + ib)
    K = (700.0, 700.0, 600.0, 180.0)
    r = Run(api, ma, ia, 3, 0.2, caps=caps)
    B = 3
    full = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    oo = [full((B, caps[0][2]), torch.uint8), full((B, caps[0][1]), torch.uint8), full((B, caps[0][1]), torch.int32), full((B,), torch.int32),
          full((B, caps[0][2]), torch.float64), full((B,), torch.int32), full((B,), torch.int32), full((B,), torch.int32)]

    def step():
        r.enqueue()
        r.h.optimize_batch(*[r.d[k].data_ptr() for k in TABLE_ARGS], B, K, *[t.data_ptr() for t in oo])

    def load(maps, inss):
        r.host = br.pack_batch(maps, *r.caps)
        r.inp = mi.pack_inputs(inss, r.feat_cap, r.prior_cap, r.outlier_cap)
        r.restore()
        with torch.cuda.stream(r.stream):
            for t in oo:                                                    # the optimise's reports keep their bytes beyond the counts
                t.zero_()

    def read():
        out = r.results()
        out.update({"opt%d" % i: t.cpu().numpy() for i, t in enumerate(oo)})
        return out

    r.stream.wait_stream(torch.cuda.current_stream())
    load(mb, ib); step(); eager_b = read()
    load(ma, ia); step(); eager_a = read()
    assert not _same(eager_a["n_obs"], eager_b["n_obs"]) and not _same(r.host["n_mp"], br.pack_batch(mb, *r.caps)["n_mp"])
    load(ma, ia)
    r.stream.synchronize()
    g = api.StepGraph.record(r.stream.cuda_stream, [], step)
    assert g.node_count() >= 4
    for maps, inss, want in ((mb, ib, eager_b), (ma, ia, eager_a)):
        load(maps, inss)
        g.launch(r.stream.cuda_stream)
        got = read()
        for k in got:
            assert _same(got[k], want[k]), k
        for i in range(3):
            check_insert_only = Run(api, [maps[i]], [inss[i]], 3, 0.2, caps=caps)
            one = check_insert_only()
            check_item(check_insert_only, check_insert_only.host, one, 0, maps[i], inss[i])
            assert _same(one["removed_kf_id"][0], got["removed_kf_id"][i]) and _same(one["feat_row"][0], got["feat_row"][i])
