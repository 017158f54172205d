"""The archive as myslam_loop_correct_batch's tables (csrc/map_archive.hip: k_map_loop_inputs, k_map_write_backend, k_map_feature_slots): items of
tests/loop_correct_ref.build_item (40 key-frames, 2 loops, 10 active, 200 points) are loaded into an archive together with matching back-end tables;
loop_inputs_batch's six outputs must be loop_correct_ref.pack's arrays exactly, the corrector run on the archive's own tables must give byte for
byte what it gives on the packed arrays (that call is checked against the oracle in tests/test_gpu_loop_correct.py), write_backend_batch must bring
the results to the selected items' back-end rows and feature_slots_batch must be a numpy search."""
import numpy as np
import pytest

import backend_ref as br
import loop_correct_ref as R
from test_gpu_loop_correct import Run as CorrectRun

pytestmark = pytest.mark.gpu

CAPS = dict(kf_cap=48, edge_cap=56, active_cap=12, point_cap=230)
BE_CAPS = (10, 120, 400)                                                    # the back end's kf_cap, mp_cap, obs_cap
KF_ID = lambda row: 4 + 3 * row                                             # ids with gaps
MP_ID = lambda slot: 1000 + 7 * slot


def archive_and_backend(item):
    """-> (the arguments of MapArchive.load, the back end's tables unpadded) for one item: every point with first_active >= 0 is an active map point
    whose first ACTIVE row is on that active key-frame, some behind a row of a key-frame that left the window; first_kf -1 = an erased point"""
    n, npt = item["n"], len(item["points"])
    rng = np.random.default_rng(npt + n)
    state = np.where((item["first_kf"] < 0), 2, np.where(rng.uniform(size=npt) < 0.1, 1, 0)).astype(np.uint8)
    load = dict(kf_id=np.array([KF_ID(i) for i in range(n)], np.int64), kf_pose=item["poses"], edge_v0=item["e0"], edge_v1=item["e1"], meas=item["meas"],
                mp_id=np.array([MP_ID(s) for s in range(npt)], np.int64), mp_pos=item["points"], mp_first_kf=np.maximum(item["first_kf"], -1), mp_state=state)
    act = [s for s in range(npt) if item["first_active"][s] >= 0]
    obs_mp, obs_kf, obs_flags = [], [], []
    for m, s in enumerate(act):
        if s % 3 == 0:                                                      # not ACTIVE, in front of the first ACTIVE row
            obs_mp.append(m); obs_kf.append(-1); obs_flags.append(0)
        fa = int(item["first_active"][s])
        for k in range(fa, min(fa + 1 + s % 3, len(item["active"]))):
            obs_mp.append(m); obs_kf.append(k); obs_flags.append(br.ACTIVE | (br.OUTLIER if (s + k) % 11 == 0 else 0))
    be = dict(kf_id=np.array([KF_ID(r) for r in item["active"]], np.int64), kf_pose=item["poses"][item["active"]] + 0.5,
              mp_id=np.array([MP_ID(s) for s in act], np.int64), mp_pos=item["points"][act] - 0.25, obs_mp=np.array(obs_mp, np.int32),
              obs_kf=np.array(obs_kf, np.int32), obs_flags=np.array(obs_flags, np.uint8))
    return load, be


def pad(bes):
    kc, mc, oc = BE_CAPS
    B = len(bes)
    t = dict(kf_id=np.full((B, kc), -77, np.int64), kf_pose=np.full((B, kc, 7), -7.5), n_kf=np.zeros(B, np.int32), mp_id=np.full((B, mc), -88, np.int64),
             mp_pos=np.full((B, mc, 3), -8.5), n_mp=np.zeros(B, np.int32), obs_mp=np.full((B, oc), -99, np.int32), obs_kf=np.full((B, oc), -98, np.int32),
             obs_flags=np.full((B, oc), 0xDD, np.uint8), n_obs=np.zeros(B, np.int32))
    for b, x in enumerate(bes):
        for k, cnt in (("kf_id", "n_kf"), ("kf_pose", "n_kf"), ("mp_id", "n_mp"), ("mp_pos", "n_mp"), ("obs_mp", "n_obs"), ("obs_kf", "n_obs"), ("obs_flags", "n_obs")):
            t[k][b, :len(x[k])] = x[k]; t[cnt][b] = len(x[k])
    return t


@pytest.fixture(scope="module")
def setup(api, synth, oracle):
    import torch
    items = [R.build_item(synth, oracle, 40, 2, seed=14, needed=True), R.build_item(synth, oracle, 40, 2, seed=12, needed=False),
             R.build_item(synth, oracle, 40, 2, seed=13, needed=True, verify_status=1)]
    B = len(items)
    stream = torch.cuda.Stream(); stream.wait_stream(torch.cuda.current_stream())
    h = api.MapArchive(B, CAPS["kf_cap"], CAPS["edge_cap"], CAPS["point_cap"], BE_CAPS[1], stream=stream.cuda_stream)
    pairs = [archive_and_backend(it) for it in items]
    for b, (load, _) in enumerate(pairs):
        h.load(b, **load)
    host = pad([be for _, be in pairs])
    d = {k: torch.from_numpy(v.copy()).cuda() for k, v in host.items()}
    return dict(items=items, B=B, stream=stream, h=h, host=host, d=d, pairs=pairs, packed=R.pack(items, **CAPS))


def loop_inputs(s, cur_ids, loop_ids, detect):
    import torch
    B, d, pc = s["B"], s["d"], CAPS["point_cap"]
    full = lambda shape: torch.full(shape, -4321, dtype=torch.int32, device="cuda")
    o = dict(active=full((B, CAPS["active_cap"])), n_active=full((B,)), cur=full((B,)), loop=full((B,)), first_active=full((B, pc)), first_kf=full((B, pc)),
             n_points=full((B,)))
    i = dict(cur=torch.tensor(cur_ids, dtype=torch.int64, device="cuda"), loop=torch.from_numpy(np.array(loop_ids, np.uint64).view(np.int64)).cuda(),
             det=torch.tensor(detect, dtype=torch.int32, device="cuda"))
    p = lambda t: t.data_ptr()
    s["h"].loop_inputs_batch(p(d["kf_id"]), p(d["n_kf"]), BE_CAPS[0], p(d["mp_id"]), p(d["n_mp"]), BE_CAPS[1], p(d["obs_mp"]), p(d["obs_kf"]), p(d["obs_flags"]),
                             p(d["n_obs"]), BE_CAPS[2], p(i["cur"]), p(i["loop"]), p(i["det"]), CAPS["active_cap"], B, *[p(o[k]) for k in
                             ("active", "n_active", "cur", "loop", "first_active", "first_kf", "n_points")])
    s["stream"].synchronize()
    return o, {k: v.cpu().numpy() for k, v in o.items()}


def test_loop_inputs_are_the_packed_arrays(setup):
    s, items, t = setup, setup["items"], setup["packed"]
    cur = [KF_ID(it["cur"]) for it in items]; loop = [KF_ID(it["loop"]) for it in items]
    _, got = loop_inputs(s, cur, loop, [0, 0, 0])
    for b, it in enumerate(items):
        na, npt = len(it["active"]), len(it["points"])
        assert got["n_active"][b] == t["n_active"][b] == na and got["n_points"][b] == t["n_points"][b] == npt
        assert np.array_equal(got["active"][b, :na], t["active"][b, :na]) and (got["active"][b, na:] == -4321).all()
        assert got["cur"][b] == t["cur"][b] and got["loop"][b] == t["loop"][b]
        assert np.array_equal(got["first_active"][b, :npt], t["first_active"][b, :npt]) and (got["first_active"][b, npt:] == -4321).all()
        assert np.array_equal(got["first_kf"][b, :npt], np.maximum(t["first_kf"][b, :npt], -1)) and (got["first_kf"][b, npt:] == -4321).all()
        assert (it["first_active"] >= 0).sum() > 40 and (it["first_kf"] < 0).sum() > 0
    # no candidate, an id the map does not hold, no key-frame this turn
    _, got = loop_inputs(s, [cur[0], cur[1], -1], [loop[0], 5, loop[2]], [1, 0, 0])
    assert list(got["loop"]) == [-1, -1, -1] and list(got["cur"]) == [items[0]["cur"], items[1]["cur"], -1]
    assert got["n_active"][2] == 0 and got["n_points"][2] == 0 and (got["first_kf"][2] == -4321).all()


def test_corrector_on_the_archive_equals_the_packed_call_then_write_back_and_slots(api, setup):
    import torch
    s, items, t, h, B = setup, setup["items"], setup["packed"], setup["h"], setup["B"]
    ref = CorrectRun(api, {k: v.copy() for k, v in t.items()}, CAPS)()
    assert list(ref["status"]) == [R.DONE, R.NOT_NEEDED, R.SKIPPED]
    o, _ = loop_inputs(s, [KF_ID(it["cur"]) for it in items], [KF_ID(it["loop"]) for it in items], [0, 0, 0])
    v = h.view()
    lc = api.LoopCorrector(B, CAPS["kf_cap"], CAPS["edge_cap"], CAPS["active_cap"], CAPS["point_cap"], stream=s["stream"].cuda_stream)
    corrected = torch.from_numpy(t["corrected"].copy()).cuda(); verify = torch.from_numpy(t["verify_status"].copy()).cuda()
    chi2 = torch.zeros(B, dtype=torch.float64, device="cuda"); iters = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.zeros(B, dtype=torch.int32, device="cuda")
    s["stream"].wait_stream(torch.cuda.current_stream())
    p = lambda x: x.data_ptr()
    lc.correct_batch(v.kf_pose, v.n_kf, p(o["active"]), p(o["n_active"]), p(o["cur"]), p(o["loop"]), p(corrected), p(verify), v.edge_v0, v.edge_v1, v.meas,
                     v.n_edges, v.mp_pos, p(o["n_points"]), p(o["first_active"]), p(o["first_kf"]), B, 1.0, 20, p(chi2), p(iters), p(st))
    s["stream"].synchronize()
    assert np.array_equal(st.cpu().numpy(), ref["status"]) and chi2.cpu().numpy().tobytes() == ref["chi2"].tobytes()
    assert np.array_equal(iters.cpu().numpy(), ref["iters"])
    arch = [h.get(b) for b in range(B)]
    for b, it in enumerate(items):
        a, n, npt = arch[b], it["n"], len(it["points"])
        E = int(ref["n_edges"][b])
        assert len(a["edge_v0"]) == E == len(it["e0"]) + (0 if b == 2 else 1)
        assert a["kf_pose"].tobytes() == ref["poses"][b, :n].tobytes() and a["mp_pos"].tobytes() == ref["points"][b, :npt].tobytes()
        assert a["meas"].tobytes() == ref["meas"][b, :E].tobytes() and np.array_equal(a["edge_v0"], ref["e0"][b, :E]) and np.array_equal(a["edge_v1"], ref["e1"][b, :E])
    assert arch[0]["kf_pose"].tobytes() != items[0]["poses"].tobytes()       # the DONE item moved
    # write-back: items 0 and 2 selected
    d, host = s["d"], s["host"]
    sel = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    h.write_backend_batch(p(d["kf_id"]), p(d["kf_pose"]), p(d["n_kf"]), BE_CAPS[0], p(d["mp_id"]), p(d["mp_pos"]), p(d["n_mp"]), BE_CAPS[1], p(sel), B)
    s["stream"].synchronize()
    kp, mp = d["kf_pose"].cpu().numpy(), d["mp_pos"].cpu().numpy()
    assert kp[1].tobytes() == host["kf_pose"][1].tobytes() and mp[1].tobytes() == host["mp_pos"][1].tobytes()
    for b in (0, 2):
        nk, nm = int(host["n_kf"][b]), int(host["n_mp"][b])
        rows = items[b]["active"]; slots = [(int(i) - 1000) // 7 for i in host["mp_id"][b, :nm]]
        assert kp[b, :nk].tobytes() == arch[b]["kf_pose"][rows].tobytes() and mp[b, :nm].tobytes() == arch[b]["mp_pos"][slots].tobytes()
        assert kp[b, nk:].tobytes() == host["kf_pose"][b, nk:].tobytes() and mp[b, nm:].tobytes() == host["mp_pos"][b, nm:].tobytes()
    # feature -> archive slot: alive, outlier-listed, erased, absent and no id
    feat_cap = 300
    rng = np.random.default_rng(3)
    ids = np.full((B, feat_cap), -66, np.int64); nf = np.array([300, 257, 0], np.int32)
    want = np.full((B, feat_cap), -4321, np.int32)
    for b in range(B):
        a = arch[b]
        pool = np.r_[a["mp_id"], a["mp_id"] + 1, [-1, -1, 5, 10 ** 12]]
        ids[b, :nf[b]] = rng.choice(pool, nf[b])
        at = np.searchsorted(a["mp_id"], ids[b, :nf[b]])
        hit = (at < len(a["mp_id"])) & (a["mp_id"][np.minimum(at, len(a["mp_id"]) - 1)] == ids[b, :nf[b]])
        want[b, :nf[b]] = np.where(hit & (a["mp_state"][np.minimum(at, len(a["mp_id"]) - 1)] != 2), at, -1)
    d_ids, d_nf = torch.from_numpy(ids).cuda(), torch.from_numpy(nf).cuda()
    out = torch.full((B, feat_cap), -4321, dtype=torch.int32, device="cuda")
    s["stream"].wait_stream(torch.cuda.current_stream())
    h.feature_slots_batch(p(d_ids), p(d_nf), feat_cap, B, p(out))
    s["stream"].synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, want) and (want[0] >= 0).sum() > 50 and (want[0] == -1).sum() > 50
