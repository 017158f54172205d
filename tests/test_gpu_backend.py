"""myslam_backend_optimize_batch (csrc/backend.hip): Backend::OptimizeActiveMap (src/backend.cpp:126-266) for a batch of active maps in device tables.
The flatten kernel against the library's host function (bytes), the solve against myslam_ba_optimize_active_map_batch on the same flat windows (bits)
and against the oracle (tests/test_gpu_ba.py's bars), the write-back against tests/backend_ref.py's literal walk fed the device's own flags and solved
values (bytes), and the call's contract: statuses, untouched bytes, slot independence, chaining, graph recording, capacities."""
import numpy as np
import pytest

import backend_ref as br

pytestmark = pytest.mark.gpu

CHI2_TH = 5.991
OUT_FILL = dict(obs_report=0xCC, mp_report=0xCB, new_outlier=-55, n_new=-56, obs_chi2=-3.25, rounds=-57, n_out=-58, status=-59)
IN_OUT = br.TABLES + ("n_kf", "n_mp", "n_obs")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Run:
    """the tables of one batch on the device, one call, everything read back"""

    def __init__(self, api, tables, K, caps, handle=None, rounds=5):
        import torch
        self.torch, self.api, self.K, self.caps, self.rounds = torch, api, K, caps, rounds
        self.B = len(tables["n_kf"])
        self.host = {k: v.copy() for k, v in tables.items()}
        self.d = {k: torch.from_numpy(v.copy()).cuda() for k, v in tables.items()}
        kf_cap, mp_cap, obs_cap = caps
        B = self.B
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        self.o = dict(obs_report=full((B, obs_cap), OUT_FILL["obs_report"], torch.uint8), mp_report=full((B, mp_cap), OUT_FILL["mp_report"], torch.uint8),
                      new_outlier=full((B, mp_cap), OUT_FILL["new_outlier"], torch.int32), n_new=full((B,), OUT_FILL["n_new"], torch.int32),
                      obs_chi2=full((B, obs_cap), OUT_FILL["obs_chi2"], torch.float64), rounds=full((B,), OUT_FILL["rounds"], torch.int32),
                      n_out=full((B,), OUT_FILL["n_out"], torch.int32), status=full((B,), OUT_FILL["status"], torch.int32))
        self.stream = torch.cuda.Stream()
        self.h = handle or api.Backend(B, kf_cap, mp_cap, obs_cap)
        self.h.set_stream(self.stream.cuda_stream)

    def restore(self):
        with self.torch.cuda.stream(self.stream):
            for k in IN_OUT:
                self.d[k].copy_(self.torch.from_numpy(self.host[k]))
            for k, v in self.o.items():
                v.fill_(OUT_FILL[k])

    def enqueue(self, batch=None):
        d, o = self.d, self.o
        self.h.optimize_batch(*[d[k].data_ptr() for k in ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags",
                                                            "obs_uv", "obs_tag", "n_obs")], self.B if batch is None else batch, self.K,
                              *[o[k].data_ptr() for k in ("obs_report", "mp_report", "new_outlier", "n_new", "obs_chi2", "rounds", "n_out", "status")],
                              rounds=self.rounds)

    def results(self):
        self.stream.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.d.items()}
        out.update({k: v.cpu().numpy() for k, v in self.o.items()})
        return out

    def __call__(self):
        self.stream.wait_stream(self.torch.cuda.current_stream())
        self.enqueue()
        return self.results()


def caps_of(maps, slack=(0, 5, 17)):
    t = [br.pack(m) for m in maps]
    return (max(len(x["kf_id"]) for x in t) + slack[0], max(len(x["mp_id"]) for x in t) + slack[1], max(len(x["obs_mp"]) for x in t) + slack[2])


def run(api, maps, K, caps=None, **kw):
    caps = caps or caps_of(maps)
    r = Run(api, br.pack_batch(maps, *caps), K, caps, **kw)
    return r, r()


def device_solve(h, b):
    """the walk's solve = what the device's own solve left for item b"""
    def solve(poses, pts, ep, el, eo, fixed):
        p2, x2, chi, out, rounds, nout = h.debug_solved(b)
        assert len(p2) == len(poses) and len(x2) == len(pts) and len(chi) == len(ep)
        return p2, x2, chi, out, rounds, nout
    return solve


def check_item(inp, out, b, m_in, rep, m_after, caps):
    """item b of a call's outputs `out` (inputs `inp`) against the walk's report `rep` and the map `m_after` it left: bytes"""
    want = br.pack(m_after)
    old = {"n_kf": int(inp["n_kf"][b]), "n_mp": int(inp["n_mp"][b]), "n_obs": int(inp["n_obs"][b])}
    new = {"n_kf": len(want["kf_id"]), "n_mp": len(want["mp_id"]), "n_obs": len(want["obs_mp"])}
    assert out["status"][b] == rep["status"] == br.DONE
    for c in ("n_kf", "n_mp", "n_obs"):
        assert out[c][b] == new[c] <= old[c], c
    for k in br.TABLES:
        c = br._COUNT_OF[k]
        assert _same(out[k][b, :new[c]], want[k]), (b, k)
        assert _same(out[k][b, new[c]:], inp[k][b, new[c]:]), (b, k, "rows from the new count on keep their bytes")      # old rows and the sentinels behind
    n_mp, n_obs = old["n_mp"], old["n_obs"]
    assert _same(out["obs_report"][b, :n_obs], rep["obs_report"]) and _same(out["mp_report"][b, :n_mp], rep["mp_report"])
    assert _same(out["obs_chi2"][b, :n_obs], rep["obs_chi2"])
    nn = len(rep["new_outlier"])
    assert out["n_new"][b] == nn and out["new_outlier"][b, :nn].tolist() == rep["new_outlier"]
    assert (out["rounds"][b], out["n_out"][b]) == (rep["rounds"], rep["n_outlier_edges"])
    assert (out["obs_report"][b, n_obs:] == OUT_FILL["obs_report"]).all() and (out["mp_report"][b, n_mp:] == OUT_FILL["mp_report"]).all()
    assert (out["obs_chi2"][b, n_obs:] == OUT_FILL["obs_chi2"]).all() and (out["new_outlier"][b, nn:] == OUT_FILL["new_outlier"]).all()


def check_against_walk(r, inp, out, maps):
    reps = []
    for b, m in enumerate(maps):
        after = m.clone()
        rep = br.walk(after, device_solve(r.h, b))
        check_item(inp, out, b, m, rep, after, r.caps)
        reps.append((rep, after))
    return reps


def untouched(inp, out, b):
    return all(_same(out[k][b], inp[k][b]) for k in IN_OUT)


# ---------------------------------------------------------------------------------------------------------------------------------------------
SEEDS = [0x300, 0x301, 0x302, 0x303, 0x304]


@pytest.fixture(scope="module")
def five(api, synth):
    made = [br.make_map(synth, s, n_kf=6, n_mp=60) for s in SEEDS]
    maps, K = [x[0] for x in made], made[0][1]
    r, out = run(api, maps, K)
    flats = [r.h.debug_flat(b) for b in range(len(maps))]
    solved = [r.h.debug_solved(b) for b in range(len(maps))]
    return dict(maps=maps, K=K, r=r, inp=r.host, out=out, flats=flats, solved=solved, kinds=[x[2] for x in made])


def test_flatten_is_the_host_functions(api, five):
    for m, flat in zip(five["maps"], five["flats"]):
        args, active_rows = br.host_flatten_args(m)
        host = api.ba_flatten_window(*args)
        assert br.same_flat(flat, host, active_rows)
        assert len(flat["edge_src"]) > 100 and len(flat["edge_src"]) < len(br.rows_of(m))


def _flat_inputs(m, flat):
    t = br.pack(m)
    return t["kf_pose"][flat["pose_src"]], t["mp_pos"][flat["pt_src"]]


def test_solve_is_the_batch_entry_points_on_the_same_windows(api, five):
    import torch
    kf_cap, mp_cap, obs_cap = five["r"].caps
    W = len(five["maps"])
    poses = np.zeros((W, kf_cap, 7)); pts = np.zeros((W, mp_cap, 3)); ep = np.zeros((W, obs_cap), np.int32); el = np.zeros((W, obs_cap), np.int32)
    obs = np.zeros((W, obs_cap, 2)); fixed = np.zeros((W, mp_cap), np.uint8); sizes = np.zeros((W, 3), np.int32)
    for w, (m, f) in enumerate(zip(five["maps"], five["flats"])):
        p, x = _flat_inputs(m, f)
        P, L, E = len(p), len(x), len(f["edge_pose"])
        poses[w, :P] = p; pts[w, :L] = x; ep[w, :E] = f["edge_pose"]; el[w, :E] = f["edge_pt"]; obs[w, :E] = f["edge_obs"]; fixed[w, :L] = f["fixed"]
        sizes[w] = (P, L, E)
    d = [torch.from_numpy(a).cuda() for a in (poses, pts, ep, el, obs, fixed, sizes)]
    scratch = torch.zeros(W * obs_cap * 18, dtype=torch.float64, device="cuda")
    chi = torch.zeros(W, obs_cap, dtype=torch.float64, device="cuda"); out = torch.zeros(W, obs_cap, dtype=torch.uint8, device="cuda")
    rd = torch.zeros(W, dtype=torch.int32, device="cuda"); no = torch.zeros(W, dtype=torch.int32, device="cuda"); st = torch.ones(W, dtype=torch.int32, device="cuda")
    api.ba_optimize_active_map_batch(*[t.data_ptr() for t in d], W, kf_cap, mp_cap, obs_cap, five["K"], CHI2_TH, CHI2_TH, 5, 10, scratch.data_ptr(),
                                     chi.data_ptr(), out.data_ptr(), rd.data_ptr(), no.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    for w, (sp, sx, schi, sout, srounds, snout) in enumerate(five["solved"]):
        P, L, E = sizes[w]
        assert _same(d[0][w, :P].cpu().numpy(), sp) and _same(d[1][w, :L].cpu().numpy(), sx)
        assert _same(chi[w, :E].cpu().numpy(), schi) and _same(out[w, :E].cpu().numpy(), sout)
        assert (int(rd[w]), int(no[w])) == (srounds, snout)
        # and the call's own outputs carry them: chi2 by row, the flags as report 1, the poses in the table
        o = five["out"]
        assert _same(o["obs_chi2"][w][five["flats"][w]["edge_src"]], schi)
        assert np.array_equal(o["obs_report"][w][five["flats"][w]["edge_src"]] == 1, sout != 0)
        assert _same(o["kf_pose"][w, :P], sp) and (o["rounds"][w], o["n_out"][w]) == (srounds, snout)


def test_solve_matches_the_oracle(oracle, five):
    for m, f, (sp, sx, schi, sout, srounds, snout) in zip(five["maps"], five["flats"], five["solved"]):
        p, x = _flat_inputs(m, f)
        rp, rx, rchi, rout, rr, rn = oracle.ba_optimize_active_map(p, x, f["edge_pose"], f["edge_pt"], f["edge_obs"], f["fixed"], five["K"])
        assert not (np.abs(rchi - CHI2_TH) < 1e-6).any()                 # the seeds: no oracle edge sits on the threshold, so EVERY flag is compared
        assert (srounds, snout) == (rr, rn)
        assert np.allclose(sp, rp, rtol=1e-7, atol=1e-8) and np.allclose(sx, rx, rtol=1e-7, atol=1e-7)
        assert np.allclose(schi, rchi, rtol=1e-6, atol=1e-9)
        assert np.array_equal(sout, rout)


def test_table_surgery_is_the_walk(five):
    reps = check_against_walk(five["r"], five["inp"], five["out"], five["maps"])
    inp, out = five["inp"], five["out"]
    fixed = new_out = old_out = leaves = kept_removed = 0
    for b, ((rep, after), f) in enumerate(zip(reps, five["flats"])):
        n_mp, n_obs = int(inp["n_mp"][b]), int(inp["n_obs"][b])
        mpr, obr, omp = out["mp_report"][b, :n_mp], out["obs_report"][b, :n_obs], inp["obs_mp"][b, :n_obs]
        fixed += int(f["fixed"].sum())
        new_out += int(out["n_new"][b])
        old_out += int(((inp["mp_outlier"][b, :n_mp] != 0) & (mpr == 2)).sum())
        leaves += int((mpr == 1).sum())
        kept_removed += int(((obr == 1) & (mpr[omp] == 0)).sum())
        assert (mpr[out["new_outlier"][b, :out["n_new"][b]]] == 2).all() and (out["mp_outlier"][b, :out["n_mp"][b]] == 0).all()
    assert fixed and new_out and old_out and leaves and kept_removed, (fixed, new_out, old_out, leaves, kept_removed)


def test_shapes(api, synth):
    # one key-frame, one map point, one row
    m = br.Map(); m.kfs[4] = np.array([0, 0, 0, 1, 0, 0, 0.0])
    mp = br.MapPoint(9, [0.5, -0.25, 12.0]); o = br.Obs(4, 650.0, 170.0, False, 77); mp.obs.append(o); mp.active_obs.append(o); m.mps[9] = mp
    K = br.make_map(synth, 1, n_kf=2, n_mp=3)[1]
    r, out = run(api, [m], K, caps=(1, 1, 1))
    assert r.h.debug_flat(0)["edge_src"].tolist() == [0]
    check_against_walk(r, r.host, out, [m])
    # counts exactly at the caps
    m, K, _ = br.make_map(synth, 0x311, n_kf=5, n_mp=50)
    caps = caps_of([m], slack=(0, 0, 0))
    r, out = run(api, [m], K, caps=caps)
    assert (r.host["n_kf"][0], r.host["n_mp"][0], r.host["n_obs"][0]) == caps
    check_against_walk(r, r.host, out, [m])
    # 10 key-frames x 600 map points: more than two passes of the 512-thread block over rows and map points, removed rows in every chunk
    m, K, _ = br.make_map(synth, 0x312, n_kf=10, n_mp=600, outlier_frac=0.08)
    r, out = run(api, [m], K)
    n_mp, n_obs = int(r.host["n_mp"][0]), int(r.host["n_obs"][0])
    assert n_mp > 1024 // 2 + 64 and n_obs > 2 * 512
    for c in range(0, n_obs, 512):
        assert (out["obs_report"][0, c:min(c + 512, n_obs)] == 1).any() and (out["obs_report"][0, c:min(c + 512, n_obs)] == 2).any()
    for c in range(0, n_mp, 512):
        assert (out["mp_report"][0, c:min(c + 512, n_mp)] != 0).any()
    check_against_walk(r, r.host, out, [m])


def test_counts_around_the_block_size(api, synth):
    """n map points with one ACTIVE row each on one key-frame, n = 511, 512, 513: the edge of the 512-thread block's chunk in the edge and landmark
    scans of the flatten and in both compactions of the write-back.  Every fifth map point is an input outlier, so map points and rows on both sides
    of the edge move down by a different number of places."""
    K = br.make_map(synth, 1, n_kf=2, n_mp=3)[1]
    sizes = (511, 512, 513)
    maps = []
    for n in sizes:
        rng = np.random.default_rng(n)
        m = br.Map(); m.kfs[4] = np.array([0, 0, 0, 1, 0, 0, 0.0])
        for j in range(n):
            pos = np.array([rng.uniform(-3, 3), rng.uniform(-1, 1), rng.uniform(8, 20)])
            mp = br.MapPoint(100 + 3 * j, pos, outlier=j % 5 == 2)
            o = br.Obs(4, K[0] * pos[0] / pos[2] + K[2], K[1] * pos[1] / pos[2] + K[3], False, 1000 + j)
            mp.obs.append(o); mp.active_obs.append(o); m.mps[mp.id] = mp
            if mp.outlier:
                m.outlier_list.append(mp.id)
        maps.append(m)
    r, out = run(api, maps, K)
    assert [(int(r.host["n_mp"][b]), int(r.host["n_obs"][b])) for b in range(3)] == [(n, n) for n in sizes]
    check_against_walk(r, r.host, out, maps)
    for b, n in enumerate(sizes):
        left = n - len(range(2, n, 5))
        assert out["n_mp"][b] == out["n_obs"][b] == left and len(r.h.debug_flat(b)["edge_src"]) == left
        assert (out["mp_report"][b, :n] == np.where(np.arange(n) % 5 == 2, 2, 0)).all() and (out["obs_report"][b, :n] == out["mp_report"][b, :n]).all()


def _bad_cases(good, K, synth):
    """name -> (mutation of the packed tables of item 1, expected status)"""
    def set_(name, idx, val):
        def f(t):
            t[name][(1,) + tuple(np.atleast_1d(idx))] = val
        return f

    p = br.pack(good)
    n_kf, n_mp, n_obs = len(p["kf_id"]), len(p["mp_id"]), len(p["obs_mp"])
    act = int(np.nonzero(p["obs_flags"] & br.ACTIVE)[0][5])
    mid = n_obs // 2
    while p["obs_mp"][mid] == p["obs_mp"][mid - 1]:
        mid += 1
    cases = {
        "n_kf negative": set_("n_kf", (), -1), "n_mp beyond its cap": set_("n_mp", (), 10 ** 6), "n_obs beyond its cap": set_("n_obs", (), 10 ** 6),
        "n_obs negative": set_("n_obs", (), -3),
        "kf ids equal": set_("kf_id", 2, int(p["kf_id"][1])), "mp ids descending": set_("mp_id", 7, int(p["mp_id"][6]) - 1),
        "obs_mp decreasing": set_("obs_mp", mid, int(p["obs_mp"][mid - 1]) - 1),
        "obs_mp >= n_mp": set_("obs_mp", n_obs - 1, n_mp), "obs_kf >= n_kf": set_("obs_kf", 3, n_kf), "obs_kf < -1": set_("obs_kf", 3, -2),
        "ACTIVE row of a key-frame that left": set_("obs_kf", act, -1),
    }
    return cases


def test_statuses_leave_the_item_alone_and_the_neighbours_as_they_were(api, synth, five):
    g0, g1 = five["maps"][0], five["maps"][1]
    K = five["K"]
    bad_src = five["maps"][2]
    caps = caps_of([g0, g1, bad_src], slack=(0, 6, 19))
    _, pair = run(api, [g0, g1], K, caps=caps)
    h = api.Backend(3, *caps)

    def go(tables, want, name):
        r = Run(api, tables, K, caps, handle=h)
        out = r()
        assert out["status"].tolist() == [br.DONE, want, br.DONE], name
        assert untouched(r.host, out, 1), name
        cm, co = min(max(int(r.host["n_mp"][1]), 0), caps[1]), min(max(int(r.host["n_obs"][1]), 0), caps[2])
        assert not out["obs_report"][1, :co].any() and not out["mp_report"][1, :cm].any() and not out["obs_chi2"][1, :co].any(), name
        assert (out["obs_report"][1, co:] == OUT_FILL["obs_report"]).all() and (out["mp_report"][1, cm:] == OUT_FILL["mp_report"]).all(), name
        assert (out["rounds"][1], out["n_out"][1], out["n_new"][1]) == (0, 0, 0) and (out["new_outlier"][1] == OUT_FILL["new_outlier"]).all(), name
        for slot, ref in ((0, 0), (2, 1)):                         # the good ones equal their results from a batch without the bad item
            for k in out:
                assert _same(out[k][slot], pair[k][ref]), (name, slot, k)

    for name, mutate in _bad_cases(bad_src, K, synth).items():
        t = br.pack_batch([g0, bad_src, g1], *caps)
        mutate(t)
        go(t, br.INVALID, name)
    lonely = bad_src.clone()                                       # a map point that is no outlier and has no observation (chain.py:589)
    lonely.mps[5] = br.MapPoint(5, [0, 0, 9.0])
    go(br.pack_batch([g0, lonely, g1], *caps), br.INVALID, "empty segment")
    edgeless = bad_src.clone()                                     # every edge row carries OUTLIER or belongs to an outlier point: nothing to optimise
    for n, mp in enumerate(edgeless.mps.values()):
        if n % 2:
            mp.outlier = True
        else:
            for o in mp.active_obs:
                o.outlier = True
    assert br.walk(edgeless.clone(), None)["status"] == br.EMPTY
    go(br.pack_batch([g0, edgeless, g1], *caps), br.EMPTY, "edgeless")


def test_all_rounds_failed_is_reported_not_refused(api, synth):
    m, K, _ = br.make_map(synth, 5, n_kf=10, n_mp=300, outlier_frac=0.6, extras=False)
    r, out = run(api, [m], K)
    assert out["status"][0] == br.DONE and out["rounds"][0] == 5 and out["n_out"][0] > 0.5 * len(r.h.debug_flat(0)["edge_src"])
    check_against_walk(r, r.host, out, [m])


def test_slot_and_repeat(api, five):
    maps, K = five["maps"], five["K"]
    caps = five["r"].caps
    x = maps[3]
    _, a = run(api, [x, maps[0]], K, caps=caps)
    r, b = run(api, [maps[1], maps[0], maps[2], maps[4], x], K, caps=caps)
    for k in a:
        assert _same(a[k][0], b[k][4]), k
        assert _same(b[k][4], five["out"][k][3]), k
    r.restore()
    again = r()
    for k in b:
        assert _same(again[k], b[k]), k


def test_chaining(five):
    """a call's output tables go straight in as the next call's input"""
    import torch
    r = five["r"]
    r.restore()
    cur = [m.clone() for m in five["maps"]]
    r.stream.wait_stream(torch.cuda.current_stream())
    for step in range(3):
        for v, k in ((r.o[k], k) for k in r.o):
            v.fill_(OUT_FILL[k])
        torch.cuda.synchronize()
        inp = {k: v.cpu().numpy() for k, v in r.d.items()}
        r.enqueue()
        out = r.results()
        for b, m in enumerate(cur):
            rep = br.walk(m, device_solve(r.h, b))
            want = br.pack(m)
            assert out["status"][b] == rep["status"] == br.DONE
            for k in br.TABLES:
                assert _same(out[k][b, :len(want[k])], want[k]), (step, b, k)
            assert (out["n_mp"][b], out["n_obs"][b]) == (len(want["mp_id"]), len(want["obs_mp"]))
            assert _same(out["obs_report"][b, :inp["n_obs"][b]], rep["obs_report"]) and _same(out["mp_report"][b, :inp["n_mp"][b]], rep["mp_report"])
    r.restore()


def test_recorded_into_a_step_graph(api, five):
    import torch
    r = five["r"]
    assert r.h.launches_per_call() == 3
    r.restore()
    g = api.StepGraph.record(r.stream.cuda_stream, [], r.enqueue)
    assert g.node_count() >= 3
    r.restore()
    r.stream.wait_stream(torch.cuda.current_stream())
    g.launch(r.stream.cuda_stream)
    got = r.results()
    for k in got:
        assert _same(got[k], five["out"][k]), k
    r.restore()


def test_capacity_and_unsupported(api, five):
    r = five["r"]
    r.restore()
    r.stream.synchronize()
    with pytest.raises(api.MyslamError) as e:
        r.enqueue(batch=r.B + 1)
    assert e.value.code == api.ERR_CAPACITY
    out = r.results()
    for k in IN_OUT:
        assert _same(out[k], r.host[k]), k                        # nothing was enqueued
    assert (out["status"] == OUT_FILL["status"]).all()
    with pytest.raises(api.MyslamError) as e:
        api.Backend(2, api.BA_MAX_WINDOW_POSES + 1, 50, 400)
    assert e.value.code == api.ERR_UNSUPPORTED
    api.Backend(2, api.BA_MAX_WINDOW_POSES, 50, 400)
