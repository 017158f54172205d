"""Loop correction for a batch of maps on the device (myslam_loop_correct_batch through api.LoopCorrector) against the reference composition of the
one-map calls through the oracle (tests/loop_correct_ref.py).

Bars (the project's own): fused active poses atol 1e-12, fused points rtol 1e-12 / atol 1e-11 (test_loop_local_fusion); the write-back 1e-10 against
oracle.correct_map_points fed the device's own poses (test_correct_map_points); the pose graph as tests/test_gpu_pgo.py holds it — fixed rows 1e-15,
the oracle's chi2 at the device's poses equal to d_chi2 to 1e-9, chi2 to max(1e-6, 10 x the oracle's own chi2 spread) relative, poses within
5e-4 max(1, n / 200)^2 or 10 x the oracle's own spread under a 1e-13 relative perturbation of its input, equal iteration counts unless both runs sit on
the chi2 floor (1e-9 relative); the appended edge's measurement 1e-12 with the quaternion sign aligned.  Statuses, counts and every byte the call
must not touch are exact."""
import numpy as np
import pytest

import loop_correct_ref as R

pytestmark = pytest.mark.gpu

CAPS = dict(kf_cap=200, edge_cap=236, active_cap=12, point_cap=256)           # every cap above every count: sentinel slots behind each table


class Run:
    """the tables of one batch on the device, one call, the tables read back"""

    def __init__(self, api, tables, caps=CAPS, corrector=None, stream=None):
        import torch
        self.torch, self.api, self.caps = torch, api, caps
        self.B = len(tables["n_kf"])
        self.host = tables
        self.d = {k: torch.from_numpy(v).cuda() for k, v in tables.items()}
        self.chi2 = torch.full((self.B,), -1.0, dtype=torch.float64, device="cuda")
        self.iters = torch.full((self.B,), -7, dtype=torch.int32, device="cuda")
        self.status = torch.full((self.B,), -7, dtype=torch.int32, device="cuda")
        self.stream = stream or torch.cuda.Stream()
        self.lc = corrector or api.LoopCorrector(self.B, caps["kf_cap"], caps["edge_cap"], caps["active_cap"], caps["point_cap"])
        self.lc.set_stream(self.stream.cuda_stream)

    def restore(self):
        with self.torch.cuda.stream(self.stream):
            for k in R.IN_OUT:
                self.d[k].copy_(self.torch.from_numpy(self.host[k]), non_blocking=False)

    def enqueue(self, corrected=None, verify_status="own"):
        d = self.d
        vs = d["verify_status"].data_ptr() if isinstance(verify_status, str) else verify_status
        self.lc.correct_batch(d["poses"].data_ptr(), d["n_kf"].data_ptr(), d["active"].data_ptr(), d["n_active"].data_ptr(), d["cur"].data_ptr(),
                              d["loop"].data_ptr(), corrected or d["corrected"].data_ptr(), vs, d["e0"].data_ptr(), d["e1"].data_ptr(),
                              d["meas"].data_ptr(), d["n_edges"].data_ptr(), d["points"].data_ptr(), d["n_points"].data_ptr(), d["first_active"].data_ptr(),
                              d["first_kf"].data_ptr(), self.B, 1.0, 20, self.chi2.data_ptr(), self.iters.data_ptr(), self.status.data_ptr())

    def results(self):
        self.stream.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.d.items()}
        out.update(chi2=self.chi2.cpu().numpy(), iters=self.iters.cpu().numpy(), status=self.status.cpu().numpy())
        return out

    def __call__(self):
        self.stream.wait_stream(self.torch.cuda.current_stream())
        self.enqueue()
        return self.results()


def run(api, items, caps=CAPS):
    t = R.pack(items, **caps)
    return t, Run(api, t, caps)()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_untouched_beyond_counts(t, out, b, appended):
    n, E, npt = int(t["n_kf"][b]), int(t["n_edges"][b]) + (1 if appended else 0), int(t["n_points"][b])
    assert _bytes_equal(out["poses"][b, n:], t["poses"][b, n:]) and _bytes_equal(out["points"][b, npt:], t["points"][b, npt:])
    for k in ("e0", "e1", "meas"):
        assert _bytes_equal(out[k][b, E:], t[k][b, E:]), k
    for k in t:
        if k not in R.IN_OUT:
            assert _bytes_equal(out[k][b], t[k][b]), k


def check_item_untouched(t, out, b):
    for k in t:
        assert _bytes_equal(out[k][b], t[k][b]), (b, k)
    assert out["chi2"][b] == 0 and out["iters"][b] == 0


def _pose_dev(a, b):
    s = np.sign(np.sum(a[:, :4] * b[:, :4], axis=1))[:, None]
    return max(np.abs(a[:, :4] * s - b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max())


def check_appended_edge(item, ref, t, out, b):
    E = len(item["e0"])
    assert out["n_edges"][b] == E + 1 and out["e0"][b, E] == item["cur"] and out["e1"][b, E] == item["loop"]
    assert _pose_dev(out["meas"][b, E:E + 1], ref["meas"][E:E + 1]) < 1e-12
    for k in ("e0", "e1", "meas"):
        assert _bytes_equal(out[k][b, :E], t[k][b, :E])


def check_fusion(item, ref, out, b):
    act = item["active"]; fa = item["first_active"] >= 0; npt = len(item["points"])
    assert np.allclose(out["poses"][b][act], ref["fused_poses"][act], rtol=0, atol=1e-12)
    assert np.allclose(out["points"][b, :npt][fa], ref["fused_points"][fa], rtol=1e-12, atol=1e-11)


def check_pose_graph(oracle, item, edges, poses, chi2, iters, tag=""):
    """The bars of tests/test_gpu_pgo.py for the pose graph of `item` after fusion; poses = the device's.  The pose graph's reference is the oracle
    run on the state the device's pose graph started from — the item's poses with the device's own fused active rows (they are fixed, so they come
    back as fusion left them) and the device's own edge table: fusion and the appended edge are held to their own bars against the oracle
    (check_fusion, check_appended_edge), and fixed rows can be held to 1e-15 only against the input they were given."""
    n = item["n"]; fx = R.fixed_of(item)
    fused = item["poses"].copy(); fused[item["active"]] = poses[item["active"]]
    G = (fused, fx) + tuple(edges)
    rp, rchi, rit = oracle.pose_graph_optimize(*G)
    assert np.abs(poses[fx.astype(bool)] - rp[fx.astype(bool)]).max() < 1e-15, tag
    chk = oracle.pose_graph_optimize(poses, *G[1:], iters=0)[1]
    assert abs(chk - chi2) <= 1e-9 * chi2, (tag, chk, chi2)
    dev, rel = _pose_dev(poses, rp), abs(chi2 - rchi) / rchi
    print(f"LOOP-CORRECT {tag} n={n} iters={iters}/{rit} chi2={chi2:.9g} rel={rel:.2e} dev={dev:.3g}")
    if rel > 1e-6 or dev >= 5e-4 * max(1.0, n / 200.0) ** 2:
        rng = np.random.default_rng(0)
        reruns = [oracle.pose_graph_optimize(fused * (1 + 1e-13 * rng.standard_normal(fused.shape)), *G[1:]) for _ in range(4)]
        chi_spread = max(abs(r[1] - rchi) for r in reruns) / rchi
        spread = max(np.abs(r[0] - rp).max() for r in reruns)
        print(f"LOOP-CORRECT {tag} oracle spread: chi2 {chi_spread:.2e} poses {spread:.3g}")
        assert rel <= max(1e-6, 10 * chi_spread), (tag, rel, chi_spread)
        assert dev < 5e-4 * max(1.0, n / 200.0) ** 2 or dev < 10 * spread, (tag, dev, spread)
    assert iters == rit or rel <= 1e-9, (tag, iters, rit)
    return rp


def check_against_composition(oracle, item, ref, poses, chi2, tag=""):
    """the end state of the reference composition itself (the oracle from start to finish), to the pose graph's chi2 and pose bars"""
    n = item["n"]
    dev, rel = _pose_dev(poses, ref["poses"]), abs(chi2 - ref["chi2"]) / ref["chi2"]
    if rel > 1e-6 or dev >= 5e-4 * max(1.0, n / 200.0) ** 2:
        rng = np.random.default_rng(0)
        G = (ref["fused_poses"], R.fixed_of(item), ref["e0"], ref["e1"], ref["meas"])
        reruns = [oracle.pose_graph_optimize(G[0] * (1 + 1e-13 * rng.standard_normal(G[0].shape)), *G[1:]) for _ in range(4)]
        chi_spread = max(abs(r[1] - ref["chi2"]) for r in reruns) / ref["chi2"]
        spread = max(np.abs(r[0] - ref["poses"]).max() for r in reruns)
        print(f"LOOP-CORRECT {tag} against the composition: rel={rel:.2e} dev={dev:.3g}, oracle spread chi2 {chi_spread:.2e} poses {spread:.3g}")
        assert rel <= max(1e-6, 10 * chi_spread), (tag, rel, chi_spread)
        assert dev < 5e-4 * max(1.0, n / 200.0) ** 2 or dev < 10 * spread, (tag, dev, spread)


def check_done(oracle, item, ref, t, out, b, tag=""):
    assert ref["status"] == R.DONE and out["status"][b] == R.DONE, (tag, out["status"][b])
    n, npt = item["n"], len(item["points"])
    check_appended_edge(item, ref, t, out, b)
    check_fusion(item, ref, out, b)
    poses = out["poses"][b, :n]
    E1 = len(item["e0"]) + 1
    check_pose_graph(oracle, item, (out["e0"][b, :E1], out["e1"][b, :E1], out["meas"][b, :E1]), poses, float(out["chi2"][b]), int(out["iters"][b]), tag)
    check_against_composition(oracle, item, ref, poses, float(out["chi2"][b]), tag)
    old = item["poses"].copy(); old[item["active"]] = poses[item["active"]]
    kf = np.where(item["first_active"] < 0, item["first_kf"], -1).astype(np.int32)
    want = oracle.correct_map_points(old, poses, kf, ref["fused_points"])
    na = item["first_active"] < 0
    assert np.abs(out["points"][b, :npt][na] - want[na]).max() < 1e-10
    assert _bytes_equal(out["points"][b, :npt][(kf < 0) & na], item["points"][(kf < 0) & na])
    check_untouched_beyond_counts(t, out, b, True)


def check_not_needed(item, ref, t, out, b):
    assert ref["status"] == R.NOT_NEEDED and out["status"][b] == R.NOT_NEEDED
    check_appended_edge(item, ref, t, out, b)
    assert _bytes_equal(out["poses"][b], t["poses"][b]) and _bytes_equal(out["points"][b], t["points"][b])
    assert out["chi2"][b] == 0 and out["iters"][b] == 0
    check_untouched_beyond_counts(t, out, b, True)


@pytest.fixture(scope="module")
def bank(synth, oracle):
    """items and their reference compositions, built once and never changed"""
    items, refs = {}, {}

    def get(key, make):
        if key not in items:
            items[key] = make()
            refs[key] = R.reference(oracle, oracle, items[key]) if items[key]["cur"] != items[key]["loop"] else None      # a self edge has no reference
        return items[key], refs[key]
    get.items, get.refs = items, refs
    for n, loops, seed in ((60, 1, 1), (120, 2, 2), (200, 3, 3), (30, 1, 4)):
        get(("needed", n), lambda: R.build_item(synth, oracle, n, loops, seed))
    get(("small", 60), lambda: R.build_item(synth, oracle, 60, 1, 5, needed=False))
    get(("all-fixed", 11), lambda: R.build_item(synth, oracle, 11, 0, 6))
    get(("one", 1), lambda: R.build_item(synth, oracle, 1, 0, 7, n_points=5))
    for vs in (1, 2, 3):
        get(("skipped", vs), lambda: R.build_item(synth, oracle, 30, 1, 10 + vs, verify_status=vs))
    return get


MIXED = [("needed", 60), ("skipped", 1), ("needed", 120), ("small", 60), ("skipped", 2), ("needed", 200), ("one", 1), ("skipped", 3), ("all-fixed", 11),
         ("needed", 30)]


@pytest.fixture(scope="module")
def mixed(api, bank):
    """one run of the mixed batch, shared by the tests that read it"""
    return run(api, [bank.items[k] for k in MIXED])


def test_mixed_batch(api, oracle, bank, mixed):
    t, out = mixed
    for b, k in enumerate(MIXED):
        item, ref = bank.items[k], bank.refs[k]
        if k[0] in ("needed", "all-fixed"):
            check_done(oracle, item, ref, t, out, b, str(k))
            if k[0] == "all-fixed":
                assert out["iters"][b] == 0
            else:
                assert out["iters"][b] >= 1 and out["chi2"][b] < 0.5 * oracle.pose_graph_optimize(ref["fused_poses"], R.fixed_of(item), ref["e0"], ref["e1"],
                                                                                                    ref["meas"], iters=0)[1]
        elif k[0] == "small":
            check_not_needed(item, ref, t, out, b)
        elif k[0] == "skipped":
            assert out["status"][b] == R.SKIPPED
        else:                                        # one key-frame: cur == loop would be a self edge
            assert out["status"][b] == R.ERR_INVALID
    assert list(out["n_edges"]) == [len(bank.items[k]["e0"]) + (1 if k[0] in ("needed", "all-fixed", "small") else 0) for k in MIXED]


def test_nothing_else_is_touched(bank, mixed):
    """sentinels in every slot beyond a count come back bit-identical; SKIPPED and ERR_* items keep every byte; NOT_NEEDED items keep poses and
    points and gain exactly one edge"""
    t, out = mixed
    assert (t["poses"][0, 60:] == R.SENTINEL_F).all() and (t["e0"][0, 59:] == R.SENTINEL_I).all()
    assert (t["points"][:, 200:] == R.SENTINEL_F).all() and (t["first_active"][:, 200:] == R.SENTINEL_I).all() and (t["first_kf"][:, 200:] == R.SENTINEL_I).all()
    assert t["n_points"].max() == 200 < t["points"].shape[1] and t["n_kf"].max() == 200        # the sentinels are there to begin with
    for b, k in enumerate(MIXED):
        if k[0] in ("skipped", "one"):
            check_item_untouched(t, out, b)
        else:
            check_untouched_beyond_counts(t, out, b, True)
            E = len(bank.items[k]["e0"])
            assert out["n_edges"][b] == E + 1 and all(_bytes_equal(out[x][b, :E], t[x][b, :E]) for x in ("e0", "e1", "meas"))
        if k[0] == "small":
            assert _bytes_equal(out["poses"][b], t["poses"][b]) and _bytes_equal(out["points"][b], t["points"][b])


def _bad_items(bank):
    """(name, item, expected status): each breaks one rule of the contract"""
    base = bank.items[("needed", 60)]

    def mod(**kw):
        it = dict(base)
        it.update(kw)
        return it
    e0 = base["e0"].copy(); e0[7] = 60
    fk = base["first_kf"].copy(); fk[np.where(base["first_active"] < 0)[0][0]] = 60
    return [("cur-not-active", mod(cur=20), R.ERR_INVALID), ("loop-beyond", mod(loop=60), R.ERR_INVALID), ("edge-beyond", mod(e0=e0), R.ERR_INVALID),
            ("first-kf-beyond", mod(first_kf=fk), R.ERR_INVALID)]


def test_per_item_errors_among_good_neighbours(api, oracle, bank):
    good = [bank.items[("needed", 60)], bank.items[("needed", 30)], bank.items[("small", 60)]]
    full = bank.items[("needed", 120)]                              # its edge table is exactly full at edge_cap = 120 (119 chain edges + one old loop)
    caps = dict(CAPS, edge_cap=len(full["e0"]))
    bad = _bad_items(bank) + [("edge-table-full", full, R.ERR_CAPACITY)]
    order = [good[0], bad[0][1], bad[1][1], good[1], bad[2][1], bad[3][1], bad[4][1], good[2]]
    where_good = [0, 3, 7]
    t, out = run(api, order, caps)
    t0, out0 = run(api, good, caps)
    for b, g in zip(where_good, range(3)):
        for k in list(R.IN_OUT) + ["chi2", "iters", "status"]:
            assert _bytes_equal(out[k][b], out0[k][g]), (b, k)
    assert list(out["status"][where_good]) == [R.DONE, R.DONE, R.NOT_NEEDED]
    for b, want in zip([1, 2, 4, 5, 6], [x[2] for x in bad]):
        assert out["status"][b] == want, (b, out["status"][b], want)
        check_item_untouched(t, out, b)
    # a batch beyond the handle's: refused as a whole, nothing enqueued
    r = Run(api, R.pack(good, **caps), caps, corrector=api.LoopCorrector(2, caps["kf_cap"], caps["edge_cap"], caps["active_cap"], caps["point_cap"]))
    with pytest.raises(api.MyslamError) as ei:
        r()
    assert ei.value.code == api.ERR_CAPACITY
    got = r.results()
    assert all(_bytes_equal(got[k], r.host[k]) for k in r.host) and (got["status"] == -7).all()


def test_position_independence_and_determinism(api, bank):
    item = bank.items[("needed", 120)]
    others = [bank.items[k] for k in (("needed", 60), ("skipped", 1), ("small", 60), ("needed", 30), ("all-fixed", 11))]
    _, alone = run(api, [item])
    batch = others + [item] + others + [bank.items[("needed", 60)]]
    assert len(batch) == 12
    t = R.pack(batch, **CAPS)
    out1 = Run(api, t)()
    out2 = Run(api, t)()
    for k in list(R.IN_OUT) + ["chi2", "iters", "status"]:
        assert _bytes_equal(alone[k][0], out1[k][5]), k
        assert _bytes_equal(out1[k], out2[k]), k
    assert out1["status"][5] == R.DONE


def _mutations(oracle, synth, bank):
    """test_pose_graph_general_structure's mutations on the 120-key-frame item"""
    base = bank.items[("needed", 120)]
    rng = np.random.default_rng(0)
    E = len(base["e0"])
    flip = rng.uniform(size=E) < 0.4
    inv = np.stack([oracle.se3_compose(np.array([0, 0, 0, 1, 0, 0, 0.0]), m, invert_b=True) for m in base["meas"]])
    out = {}
    out["either-orientation"] = dict(base, e0=np.where(flip, base["e1"], base["e0"]).astype(np.int32), e1=np.where(flip, base["e0"], base["e1"]).astype(np.int32),
                                     meas=np.where(flip[:, None], inv, base["meas"]))
    out["duplicated-chain-edge"] = dict(base, e0=np.r_[base["e0"], base["e0"][10:11]].astype(np.int32), e1=np.r_[base["e1"], base["e1"][10:11]].astype(np.int32),
                                        meas=np.concatenate([base["meas"], base["meas"][10:11]]))
    i, j = int(base["e0"][-1]), int(base["e1"][-1])                  # synth's old loop (i, j)
    extra = oracle.se3_compose(oracle.se3_compose(base["gt"][i - 3], base["gt"][j], invert_b=True), oracle.se3_exp(0.003 * rng.standard_normal(6)))
    out["two-loops-into-one"] = dict(base, e0=np.r_[base["e0"], i - 3].astype(np.int32), e1=np.r_[base["e1"], j].astype(np.int32),
                                     meas=np.concatenate([base["meas"], extra[None]]))
    mid = (i + j) // 2                                               # an active (hence fixed) row inside the old loop, displaced like the window
    poses = base["poses"].copy(); poses[mid] = oracle.se3_compose(poses[mid], oracle.se3_exp(R.NEEDED_MOTION))
    act = np.r_[mid, base["active"]].astype(np.int32)
    fa = np.where(base["first_active"] >= 0, base["first_active"] + 1, -1).astype(np.int32)
    out["active-row-inside-old-loop"] = dict(base, poses=poses, active=act, first_active=fa,
                                             first_kf=np.where(fa >= 0, act[np.maximum(fa, 0)], base["first_kf"]).astype(np.int32))
    cut = mid + 2                                                    # the chain edge (cut, cut - 1) goes: the old loop still holds the graph together
    keep = ~((base["e0"] == cut) & (base["e1"] == cut - 1))
    assert keep.sum() == E - 1 and j < cut - 1 and cut < i
    out["no-edge-to-row-neighbour"] = dict(base, e0=base["e0"][keep], e1=base["e1"][keep], meas=base["meas"][keep])
    allact = np.arange(1, 120, dtype=np.int32)                       # every row but row 0 active: nothing is free
    fa = np.where(base["first_active"] >= 0, base["active"][np.maximum(base["first_active"], 0)] - 1, -1).astype(np.int32)
    out["every-key-frame-fixed"] = dict(base, active=allact, first_active=fa)
    return out


def test_structure_mutations_at_120_key_frames(api, oracle, synth, bank):
    muts = _mutations(oracle, synth, bank)
    names = list(muts)
    t, out = run(api, [muts[k] for k in names], dict(CAPS, active_cap=120))
    for b, k in enumerate(names):
        ref = R.reference(oracle, oracle, muts[k])
        check_done(oracle, muts[k], ref, t, out, b, k)
        if k == "every-key-frame-fixed":
            assert out["iters"][b] == 0
        else:
            assert out["iters"][b] >= 1


def test_the_separator_limit(api, oracle, synth, bank):
    base = R.build_item(synth, oracle, 120, 1, 21)
    at, over = R.add_short_loops(oracle, base, R.MAX_SEPARATORS), R.add_short_loops(oracle, base, R.MAX_SEPARATORS + 1)
    for it, want in ((at, (R.MAX_SEPARATORS, True)), (over, (R.MAX_SEPARATORS + 1, False))):
        ns, _, ok = api.loop_correct_structure(it["n"], it["active"], it["loop"], it["e0"], it["e1"])
        assert (ns, ok) == want
    t, out = run(api, [at, over, bank.items[("needed", 60)]])
    check_done(oracle, at, R.reference(oracle, oracle, at), t, out, 0, "32-separators")
    check_done(oracle, bank.items[("needed", 60)], bank.refs[("needed", 60)], t, out, 2, "neighbour")
    # one more: fused, the rest of the map untouched
    ref = R.reference(oracle, oracle, over)
    assert out["status"][1] == R.FUSED_ONLY and out["iters"][1] == 0 and out["chi2"][1] == 0
    check_appended_edge(over, ref, t, out, 1)
    check_fusion(over, ref, out, 1)
    n, npt = over["n"], len(over["points"])
    rest = np.setdiff1d(np.arange(n), over["active"]); na = over["first_active"] < 0
    assert _bytes_equal(out["poses"][1, :n][rest], over["poses"][rest]) and _bytes_equal(out["points"][1, :npt][na], over["points"][na])
    check_untouched_beyond_counts(t, out, 1, True)
    # the caller finishes with the host-pointer calls and lands on the reference composition
    fused, E1 = out["poses"][1, :n], int(out["n_edges"][1])
    e0, e1, meas = out["e0"][1, :E1], out["e1"][1, :E1], out["meas"][1, :E1]
    opt, chi2, its = api.pose_graph_optimize(fused, R.fixed_of(over), e0, e1, meas)
    rp = check_pose_graph(oracle, over, (e0, e1, meas), opt, chi2, its, "33-separators-finished-on-the-host")
    kf = np.where(na, over["first_kf"], -1).astype(np.int32)
    pts = api.correct_map_points(fused, opt, kf, out["points"][1, :npt])
    assert np.abs(pts - oracle.correct_map_points(fused, opt, kf, out["points"][1, :npt])).max() < 1e-10
    check_against_composition(oracle, over, ref, opt, chi2, "33-separators-finished-on-the-host")


def test_stream_order_behind_verify_batch(api, oracle, synth, bank):
    """verify_batch and correct_batch back to back on one stream: the corrector reads verify's d_pose7 / d_status where that call left them"""
    import torch
    keys = [("needed", 60), ("needed", 30), ("small", 60)]
    cap = 128
    K = None
    items, p3s, p2s, cnt = [], [], [], []
    for b, k in enumerate(keys):
        p3, p2, K, pose, _ = synth.pnp_problem(n=120, outlier_frac=0.2, seed=40 + b)
        item = dict(bank.items[k])
        # re-base the map's world frame so that its corrected pose is the PnP problem's pose: Tcw' = Tcw * G leaves every measurement as it is
        G = oracle.se3_compose(oracle.se3_compose(np.array([0, 0, 0, 1, 0, 0, 0.0]), item["corrected"], invert_b=True), pose)
        item["poses"] = np.stack([oracle.se3_compose(p, G) for p in item["poses"]])
        items.append(item); p3s.append(p3); p2s.append(p2); cnt.append(5 if b == 1 else 120)           # item 1: too few matches, verify gives up
    B = len(keys)
    P3 = np.zeros((B, cap, 3), np.float32); P2 = np.zeros((B, cap, 2), np.float32)
    for b in range(B):
        P3[b, :120] = p3s[b]; P2[b, :120] = p2s[b]
    t = R.pack(items, **CAPS)
    stream = torch.cuda.Stream()
    solver = api.PnPSolver(B, cap, 100, stream=stream.cuda_stream)
    r = Run(api, t, stream=stream)
    d3, d2, dc = torch.from_numpy(P3).cuda(), torch.from_numpy(P2).cuda(), torch.tensor(cnt, dtype=torch.int32, device="cuda")
    pose = torch.zeros((B, 7), dtype=torch.float64, device="cuda"); flag = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
    ninl = torch.zeros(B, dtype=torch.int32, device="cuda"); st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    solver.verify_batch(d3.data_ptr(), d2.data_ptr(), dc.data_ptr(), B, K, pose.data_ptr(), flag.data_ptr(), ninl.data_ptr(), st.data_ptr())
    r.enqueue(corrected=pose.data_ptr(), verify_status=st.data_ptr())
    out = r.results()
    vpose, vst = pose.cpu().numpy(), st.cpu().numpy()
    assert list(vst) == [api.VERIFY_CONFIRMED, api.VERIFY_FEW_MATCHES, api.VERIFY_CONFIRMED]
    t["corrected"][:] = vpose; t["verify_status"][:] = vst
    out["corrected"] = vpose; out["verify_status"] = vst          # the call read them from verify's buffers, not from the tables
    for b in range(B):
        item = dict(items[b], corrected=vpose[b], verify_status=int(vst[b]))
        ref = R.reference(oracle, oracle, item)
        if ref["status"] == R.DONE:
            check_done(oracle, item, ref, t, out, b, f"behind-verify-{b}")
        elif ref["status"] == R.NOT_NEEDED:
            check_not_needed(item, ref, t, out, b)
        else:
            assert out["status"][b] == R.SKIPPED
            check_item_untouched(t, out, b)
    assert list(out["status"]) == [R.DONE, R.SKIPPED, R.NOT_NEEDED]


def test_recorded_into_a_step_graph_and_no_device_memory_growth(api, bank):
    import torch
    items = [bank.items[k] for k in (("needed", 60), ("small", 60), ("skipped", 2), ("needed", 120))]
    t = R.pack(items, **CAPS)
    r = Run(api, t)
    eager = r()
    assert list(eager["status"]) == [R.DONE, R.NOT_NEEDED, R.SKIPPED, R.DONE]
    r.restore()
    g = api.StepGraph.record(r.stream.cuda_stream, [], r.enqueue)
    assert g.node_count() >= 1
    for _ in range(2):
        r.restore()
        r.chi2.fill_(-1); r.iters.fill_(-7); r.status.fill_(-7)
        r.stream.wait_stream(torch.cuda.current_stream())
        g.launch(r.stream.cuda_stream)
        got = r.results()
        for k in eager:
            assert _bytes_equal(got[k], eager[k]), k
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        r.restore()
        r.enqueue()
    r.stream.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 64 << 20
