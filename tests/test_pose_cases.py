"""tests/pose_cases.py proved on the oracle alone, before any GPU sees a case.  A (problem, move) pair is held at the existing
parity bars by tests/test_gpu_pose_moved.py only if it passes three checks here:

  reach      a pair that claims a branch: every output pose of the oracle takes it with |trace| > 0.25 and the winning diagonal element more than
             0.1 ahead; per solver branches 1, 2 and 3 are each reached and at least one output has raw w < 0.  d120 (trace ~ 0) claims nothing, and
             neither does skew170 for BA and pose-only: their cameras look down +z, R' = Rcw Rg^T then has x and z diagonal elements 0.06 apart or
             less whatever the seed (for PnP, whose cameras yaw by up to 0.6 rad, skew170 leads by 0.55 and 0.65 and claims 1 and 3).
  stability  the method of tests/golden/make_pose_only_weak_frame.py and test_gpu_pnp_batch._oracle_is_stable: eight seeded one-ulp perturbations
             of the observations leave flags and counts as they are and the moved-back pose (BA: poses and points) within 1e-10 — on the moved AND
             on the unmoved problem, since the metamorphic check compares the two.  Pose-only adds 48 draws (pose_cases.po_draws: one ulp of the map
             points, of the start translation, of all three) at the same 1e-10: see below.
  d_ref      |move_back(oracle(moved)) - oracle(unmoved)| is printed (pytest -s); the GPU tests compute it again and hold the device to 10 x it.

Seeds tried (a pair that failed was replaced by another seed, never by a looser bar):
  pose-only  First gate, the eight draws alone: seeds 0..39 of test_gpu_pose_only._problem at (n, bad) = (37, 3), (120, 12), (200, 20), (80, 8), (150, 30)
             gave 77 stable pairs for plain20, 40 for y135, and of the kilometre moves 6 for x180, 6 for y180, 8 for z180, 6 for skew170, 3 for d120;
             dropped among others (1, 37, 3), (21, 120, 12), (5, 200, 20) (5.6e-9 .. 1.1e-8), (0, 200, 20) under every kilometre move (8.3e-9: the tie
             of the issue), (22, 190, 10), (7, 120, 30).  The device then missed the 1e-8 / 1e-9 bar on (9, 200, 20) x y180, which had passed (4.4e-11):
             2e-8 from the oracle in t.  The oracle itself lands 1.6e-8 away when the moved map points change by one ulp (1.8e-12 m at 1e4 m, the
             size of the rounding a fused multiply-add or another summation order leaves in a camera-frame point), and 2.4e-9 under sixteen draws
             of the observations instead of eight: a late accept / reject tie that eight draws did not hit.  Hence the 48 further draws.  Under
             them NO frame of seeds 0..299 x (37, 80, 120, 200 matches) or 0..79 x 2100 matches is stable under x180, y180, z180, skew170 or d120
             with the table's translations; 113 are under y135 (450 m), and with tg scaled to 500 m 104 / 118 / 82 / 16 / 48 (seeds 0..119) are under
             the five rotations.  So the strong pairs take those rotations at 500 m (the "_near" moves), and the pairs that passed the first gate keep
             the table's own kilometres as PO_FAR, judged against the oracle's own scatter (test_gpu_pose_moved.check_po, far rule).
  BA         seeds 0..47 of synth.ba_problem at (7, 120), (4, 40), (5, 60), (6, 80) key-frames x landmarks.  Windows of 0.03 outliers are stable
             under plain20 .. y180 almost always, under z180 only at 7 x 120 (seeds 6, 8, 9, 12, ...: 7e-11 .. 9e-11; seed 3: 1.2e-10, dropped; with
             3.7-fold quaternions (3, 7, 120) leaves the gate under x180 and y180 too, 1.09e-10).  Under skew170 and d120 NO window is: |tg| of 1e4 m
             puts the window's own one-ulp scatter at 1.4e-10 .. 9e-10.  Those two rotations run with tg scaled to 500 m (skew170_near, d120_near).
             Windows that fail all five rounds: of 30 seeds x (5 x 60, 4 x 40) at 0.6 outliers one is stable under x180 (14, 4 x 40), none under
             y180 or z180, 17 under y135 (2, 5 x 60 is used).  Dropped: (9, 4, 40) (2.7e-10 unmoved), (11, 5, 60, 0.3) and (5, 6, 80, 0.6) (5e-10 .. 4e-7).
             BA keeps the eight draws: its bars (1e-7 / 1e-8) lie two decades above the gate, pose-only's atol of 1e-9 one.
  PnP        (120, 9), (65, 11), (200, 12), (63, 11): every move keeps the consensus set; none dropped.  The second stage of verify_batch is stable
             at 1e-10 for (63, 11) under y135, x180, y180, z180 and for (120, 9) under plain20; (65, 11), (200, 12), (128, 11) are not (2e-10 .. 8e-9).

The second half rehearses the GPU tests' checkers against stand-ins that wrap the oracle with one deliberate fault each: every one must be rejected.
CPU only."""
import numpy as np
import pytest

import pose_cases as PC
import tracker_cases as TC
from test_gpu_pose_moved import check_ba, check_classwise, check_neighbours, check_pnp, check_po, check_seen


@pytest.fixture(scope="module")
def R(synth, oracle):
    return PC.refs(synth, oracle)


def test_helpers_agree_with_the_textbook_forms(pkg):
    chain = pkg.chain
    rng = np.random.default_rng(5)
    qs = [TC.quat(ax, deg) for _, ax, deg, _ in PC.MOVE_SPEC] + [rng.normal(size=4) for _ in range(20)] + [np.array([1.0, 0, 0, 0]), np.array([0, 0, 1e-9, 1.0])]
    for q in qs:
        Rm = PC.R_of_q(q)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rm) - 1) < 1e-14
        assert np.abs(Rm - chain.T_of(TC.pose7(q / np.sqrt(q @ q), (0, 0, 0)))[:3, :3]).max() < 1e-15          # the package's own q -> R
        back = PC.q_of_R(Rm)
        assert back[3] >= 0 and abs(back @ back - 1) < 1e-15 and np.abs(PC.R_of_q(back) - Rm).max() < 1e-14   # the eigenvector route inverts it
        assert PC.branch_of(Rm)[0] == TC.branch_of(Rm)[0]
    for name in PC.MOVES:
        G = PC.move(name)
        p = TC.pose7(TC.quat((0.2, -1.0, 0.4), 7.0), (0.4, -0.1, 0.6))
        x = rng.uniform(-20, 20, (5, 3))
        for scale in (1.0, -1.0, 3.7):
            m = PC.move_pose(G, p, scale)
            assert abs(np.sqrt(m[:4] @ m[:4]) - abs(scale)) < 1e-14
            assert PC.pose_dist(PC.move_back(G, m), PC.canon(p)) < 1e-11                                          # 1e4 m x 1e-16
            cam = PC.move_points(G, x) @ PC.R_of_q(m[:4]).T + m[4:]                                                # camera-frame points do not change
            assert np.abs(cam - (x @ PC.R_of_q(p[:4]).T + p[4:])).max() < 1e-11
        assert np.abs(PC.points_back(G, PC.move_points(G, x)) - x).max() < 1e-11
    assert np.abs(PC.move("d120_near")[1]).max() == 500.0 and PC.branch_of(PC.R_of_q(TC.quat((1, 1, 1), 120.0)))[1] < 1e-15


def _reach(poses, claim, tag):
    out = []
    for p in poses:
        b, tr, lead = PC.branch_of(PC.R_of_q(p[:4]))
        if claim is not None:
            assert b == claim and abs(tr) > 0.25 and lead > 0.1, (tag, "does not reach branch", claim, b, tr, lead)
            out.append(b)
    return out


def _po_stable(oracle, args, ref, G, tag, pre=0, draws=None):
    """flags and count unchanged and the moved-back pose within 1e-10 over the draws (default: all 56 of pose_cases.po_draws)"""
    back, worst = PC.move_back(G, ref[0]), 0.0
    for a in (PC.po_draws(args) if draws is None else draws):
        q = oracle.pose_only_optimize(*a, pre_optimize=pre)
        assert q[2] == ref[2] and np.array_equal(q[1], ref[1]), (tag, "a one-ulp perturbation changes flags or count")
        worst = max(worst, PC.pose_dist(PC.move_back(G, q[0]), back))
    assert worst <= 1e-10, (tag, "one-ulp perturbations move the pose by", worst)
    return worst


def test_pose_only_pairs_qualify(oracle, R):
    reached, wneg = [], 0
    for key, name, scale, claim in PC.PO_PAIRS + PC.PO_BIG:
        r = R.po(key, name, scale)
        tag = f"pose-only {key} {name} x{scale}"
        q0 = r["args"][0][:4]
        assert abs(np.sqrt(q0 @ q0) - abs(scale)) < 1e-14 and (scale > 0) == (q0[3] > 0), tag                  # negated / 3.7-fold as the table says
        reached += _reach([r["ref"][0]], claim, tag)
        wneg += r["ref"][0][3] < 0
        assert r["ref"][2] == r["base"][2] and np.array_equal(r["ref"][1], r["base"][1]), (tag, "the move changes flags")
        assert r["ref"][1].sum() >= 3                                                                           # there are outliers to flag
        w = _po_stable(oracle, r["args"], r["ref"], r["G"], tag)
        r0 = R.po(key, None, 1.0)
        w0 = _po_stable(oracle, r0["args"], r0["ref"], r0["G"], tag + " unmoved")
        assert r["d_ref"] <= 1e-8, (tag, r["d_ref"])
        print(f"{tag}: branch {PC.branch_of(PC.R_of_q(r['ref'][0][:4]))}, d_ref {r['d_ref']:.1e}, one-ulp scatter {w:.1e} (unmoved {w0:.1e})")
    assert {1, 2, 3} <= set(reached) and wneg >= 1
    assert {p[1].replace("_near", "") for p in PC.PO_PAIRS} == set(PC.MOVES)                                    # every rotation of the table runs


def test_pose_only_far_pairs(oracle, R):
    """the table's own kilometre translations: each pair reaches its branch and passes the issue's gate (eight draws of the observations), none
    passes the 48 further draws — which is why they are judged against the oracle's own scatter"""
    reached, wneg = [], 0
    for key, name, scale, claim in PC.PO_FAR:
        r = R.po(key, name, scale)
        tag = f"pose-only far {key} {name} x{scale}"
        assert np.abs(r["G"][1]).max() >= 5e3, tag
        reached += _reach([r["ref"][0]], claim, tag)
        wneg += r["ref"][0][3] < 0
        assert r["ref"][2] == r["base"][2] and np.array_equal(r["ref"][1], r["base"][1]), (tag, "the move changes flags")
        w8 = _po_stable(oracle, r["args"], r["ref"], r["G"], tag, draws=list(PC.po_draws(r["args"]))[:8])
        s = R.po_scatter(key, name, scale)
        assert s is not None and 1e-10 < s < 1e-6, (tag, s)
        print(f"{tag}: branch {PC.branch_of(PC.R_of_q(r['ref'][0][:4]))}, d_ref {r['d_ref']:.1e}, scatter over eight draws {w8:.1e}, over all 56 {s:.1e}")
    assert {1, 2, 3} <= set(reached) and wneg >= 1 and {p[1] for p in PC.PO_FAR} == set(PC.MOVES[2:])
    print(f"the oracle's own scatter at kilometre offsets: {R.far_scatter():.2e}")


def _ba_stable(oracle, r, tag):
    rng = np.random.default_rng(0)
    a = r["args"]
    worst = 0.0
    for _ in range(8):
        q = oracle.ba_optimize_active_map(a[0], a[1], a[2], a[3], PC.one_ulp(rng, a[4]), a[5], a[6])
        assert q[4:] == r["ref"][4:] and np.array_equal(q[3], r["ref"][3]), (tag, "a one-ulp perturbation changes rounds, flags or count")
        worst = max(worst, PC.ba_dist(r["G"], q, r["G"], r["ref"]))
    assert worst <= 1e-10, (tag, "one-ulp perturbations move the window by", worst)
    return worst


def test_ba_pairs_qualify(oracle, R):
    reached, wneg, rounds, unmoved = [], 0, set(), {}
    for key, name, scale, claim in PC.BA_PAIRS:
        r = R.ba(key, name, scale)
        tag = f"ba {key} {name} x{scale}"
        for p in r["args"][0]:
            assert abs(np.sqrt(p[:4] @ p[:4]) - abs(scale)) < 1e-14 and (scale > 0) == (p[3] > 0), tag
        P, L, E = len(r["args"][0]), len(r["args"][1]), len(r["args"][2])
        assert 4 <= P <= 7 and 40 <= L <= 120 and E <= 900
        reached += _reach(r["ref"][0], claim, tag)
        wneg += int((r["ref"][0][:, 3] < 0).sum())
        rounds.add(r["ref"][4])
        assert r["ref"][4:] == r["base"][4:] and np.array_equal(r["ref"][3], r["base"][3]), (tag, "the move changes rounds or flags")
        # the GPU's chi2 is held to rtol 1e-6 of the oracle's (6e-6 at the threshold) and the outlier COUNT must be equal: no edge may sit that close
        assert np.abs(r["ref"][2] - PC.CHI2).min() > 1e-4, (tag, "an edge sits on the chi2 threshold", np.abs(r["ref"][2] - PC.CHI2).min())
        w = _ba_stable(oracle, r, tag)
        if key not in unmoved:
            unmoved[key] = _ba_stable(oracle, R.ba(key, None, 1.0), tag + " unmoved")
        w0 = unmoved[key]
        assert r["d_ref"] <= 1e-9, (tag, r["d_ref"])
        print(f"{tag}: branches {[PC.branch_of(PC.R_of_q(p[:4]))[0] for p in r['ref'][0]]}, rounds {r['ref'][4]}, d_ref {r['d_ref']:.1e}, "
              f"one-ulp scatter {w:.1e} (unmoved {w0:.1e})")
    assert {1, 2, 3} <= set(reached) and wneg >= 1 and rounds == {0, 5}                                       # solved windows and windows that fail every round
    assert {p[1].replace("_near", "") for p in PC.BA_PAIRS} == set(PC.MOVES)


def _pnp_one_ulp(rng, uv):
    return np.where(rng.integers(0, 2, uv.shape) == 1, np.nextafter(uv, np.float32(np.inf)), np.nextafter(uv, np.float32(-np.inf))).astype(np.float32)


def test_pnp_pairs_qualify(oracle, R):
    """PnP's observations are f32: one ulp of a pixel (at most 2^-13 px below 2048) turns a ray by 1.7e-7 rad (f = 718 px), which moves a point 45 m out
    by 8e-6 m.  Stable here means: mask and count unchanged and the pose within 1e-4 — a pose that jumps further has changed its winner."""
    reached, wneg = [], 0
    for key, name, max_t, claim in PC.PNP_PAIRS + [PC.PNP_FAR]:
        r = R.pnp(key, name, max_t)
        tag = f"pnp {key} {name} |tg| <= {max_t}"
        pw, uv, Kt = r["args"]
        rc, pose, inl, ni = r["ref"]
        assert rc == 0 and ni >= 20 and len(pw) <= 200 and pw.dtype == np.float32, tag
        far = (key, name, max_t, claim) == PC.PNP_FAR
        assert (np.abs(r["G"][1]).max() < 1000.0) != far, tag
        reached += _reach([pose], claim, tag)
        wneg += pose[3] < 0
        assert ni == r["base"][3] and np.array_equal(inl, r["base"][2]), (tag, "the move changes the consensus set")
        rng = np.random.default_rng(0)
        for _ in range(8):
            q = oracle.solve_pnp_ransac(pw, _pnp_one_ulp(rng, uv), Kt)
            assert q[0] == 0 and q[3] == ni and np.array_equal(q[2], inl) and PC.pose_dist(PC.move_back(r["G"], q[1]), PC.move_back(r["G"], pose)) < 1e-4, tag
        print(f"{tag}: branch {PC.branch_of(PC.R_of_q(pose[:4]))}, {ni} inliers, d_ref {r['d_ref']:.1e}")
    assert {1, 2, 3} <= set(reached) and wneg >= 1
    for key, name, max_t in PC.PNP_CHAIN:                                                                        # the second stage of verify_batch
        r = R.pnp(key, name, max_t)
        pw, uv, Kt = r["args"]
        chain = R.chain(key, name, max_t)
        assert chain[2] >= 10
        args = (r["ref"][1], pw.astype(np.float64), uv.astype(np.float64), Kt)
        _po_stable(oracle, args, chain, r["G"], f"chain {key} {name}", pre=1, draws=list(PC.po_draws(args))[:8])


def test_odd_inputs_are_what_their_names_say(synth, oracle):
    E, Kt = PC.pnp_edges(synth)
    for name, c in E.items():
        PC.expect_holds(oracle.solve_pnp_ransac(c["pw"], c["uv"], Kt, **c["kw"]), c, name)
        assert len(c["pw"]) <= 200
    base = oracle.pose_only_optimize(*PC.po_problem(synth, oracle, PC.PO_ODD_BASE))
    for kind in PC.PO_ODD:
        args = PC.po_odd(synth, oracle, kind)
        p, o, n = oracle.pose_only_optimize(*args)
        if kind == "behind3":
            assert np.isfinite(p).all() and np.abs(p - base[0]).max() < 1e-2 and o[[11, 50, 90]].all()
            _po_stable(oracle, args, (p, o, n), PC.IDENTITY, kind)
        else:
            assert p.tobytes() == args[0].tobytes(), (kind, "the oracle's definite answer is: pose unchanged")
    frames, counts, Kt = PC.count_rule_frames(synth, oracle)
    for (T0, pts, obs), n in zip(frames[1:], (64, 40)):
        ref = oracle.pose_only_optimize(T0, pts[:n], obs[:n], Kt)
        assert 0 < ref[1].sum() < n
        _po_stable(oracle, (T0, pts[:n], obs[:n], Kt), ref, PC.IDENTITY, f"count rule, {n} matches")
    for kind in PC.BA_ODD:
        args = PC.ba_odd(synth, kind)
        ref = oracle.ba_optimize_active_map(*args)
        assert np.isfinite(ref[0]).all() and not np.isfinite(ref[2][77])


# ---- the checkers reject faulty stand-ins --------------------------------------------------------------------------------------------
def _faulty(oracle, fault):
    """oracle.pose_only_optimize with one deliberate fault in what it hands back"""
    def solve(T0, pts, obs, Kt):
        pose, out, ni = oracle.pose_only_optimize(T0, pts, obs, Kt)
        b = PC.branch_of(PC.R_of_q(pose[:4]))[0]
        if fault == "w_sign_branch2" and b == 2:
            pose[3] = -pose[3]
        if fault == "xy_swapped_branch3" and b == 3:
            pose[[0, 1]] = pose[[1, 0]]
        if fault == "not_renormalised":
            pose[:4] *= np.sqrt(T0[:4] @ T0[:4])
        if fault == "flags_shifted":
            out = np.roll(out, 1)
        return pose, out, ni
    return solve


def test_checkers_reject_faulty_stand_ins(oracle, R):
    pairs = {p[1].replace("_near", ""): p for p in PC.PO_PAIRS[:7]}
    good = _faulty(oracle, None)
    stats = []
    for key, name, scale, claim in PC.PO_PAIRS:                       # the stand-in without a fault passes everything
        r = R.po(key, name, scale)
        stats.append(check_po(r, good(*r["args"]), good(*R.po(key, None, 1.0)["args"]), name, claim))
    check_seen(stats, "the oracle as a stand-in")
    for fault, name in (("w_sign_branch2", "y135"), ("w_sign_branch2", "y180"), ("xy_swapped_branch3", "z180"), ("not_renormalised", "x180"),
                        ("not_renormalised", "d120"), ("flags_shifted", "plain20"), ("flags_shifted", "skew170")):
        key, name, scale, claim = pairs[name]
        r = R.po(key, name, scale)
        bad = _faulty(oracle, fault)
        with pytest.raises(AssertionError):
            check_po(r, bad(*r["args"]), good(*R.po(key, None, 1.0)["args"]), fault, claim)
    with pytest.raises(AssertionError):                               # a solver that never leaves branch 0 / never writes w < 0
        check_seen([s for s in stats if s["branch"] != 3], "no branch 3")
    with pytest.raises(AssertionError):
        check_seen([dict(s, wneg=False) for s in stats], "no negative w")
    far = PC.PO_FAR[1]                                                # the far rule is no free pass: 1e-6 off, or a wrong w, is rejected
    r = R.po(*far[:3])
    check_po(r, good(*r["args"]), good(*R.po(far[0], None, 1.0)["args"]), "far", far[3], far=R.far_scatter())
    with pytest.raises(AssertionError):
        check_po(r, _faulty(oracle, "w_sign_branch2")(*r["args"]), good(*R.po(far[0], None, 1.0)["args"]), "far", far[3], far=R.far_scatter())
    with pytest.raises(AssertionError):
        off = good(*r["args"]); off[0][5] += 1e-5
        check_po(r, off, good(*R.po(far[0], None, 1.0)["args"]), "far", far[3], far=R.far_scatter())
    with pytest.raises(AssertionError):                               # a solver that is right on the moved problem but not on the unmoved one
        key, name, scale, claim = PC.PO_PAIRS[3]
        r = R.po(key, name, scale)
        off = good(*R.po(key, None, 1.0)["args"]); off[0][5] += 1e-6
        check_po(r, good(*r["args"]), off, "metamorphic", claim)
    # BA and PnP: the same two write-back faults
    key, name, scale, claim = PC.BA_BATCH[1]
    r = R.ba(key, name, scale)
    base = R.ba(key, None, 1.0)["ref"]
    check_ba(r, r["ref"], base, "ba", claim)
    bad = tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in r["ref"])
    bad[0][2, [0, 1]] = bad[0][2, [1, 0]]
    with pytest.raises(AssertionError):
        check_ba(r, bad, base, "ba x / y swapped", claim)
    bad = tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in r["ref"])
    bad[3][:] = np.roll(bad[3], 1)
    with pytest.raises(AssertionError):
        check_ba(r, bad, base, "ba flags shifted", claim)
    key, name, max_t, claim = PC.PNP_PAIRS[3]
    r = R.pnp(key, name, max_t)
    base = R.pnp(key, None, None)["ref"][1:]
    check_pnp(r, r["ref"][1:], base, "pnp", claim)
    bad = (r["ref"][1].copy(), r["ref"][2], r["ref"][3]); bad[0][3] = -bad[0][3]
    with pytest.raises(AssertionError):
        check_pnp(r, bad, base, "pnp w sign", claim)
    with pytest.raises(AssertionError):
        check_pnp(r, (r["ref"][1], np.roll(r["ref"][2], 1), r["ref"][3]), base, "pnp mask shifted", claim)


def test_neighbour_and_classwise_checkers(synth, oracle):
    """a batch stand-in (the oracle frame by frame) that lets a NaN frame disturb the frame behind it, and one that moves the pose of a NaN frame"""
    frames = [PC.po_problem(synth, oracle, PC.PO_PROBLEMS[k]) for k in ("a", "b", "c")]
    odd = PC.po_odd(synth, oracle, "nan_obs")

    def batch(items, leaky):
        res = [oracle.pose_only_optimize(*f) for f in items]
        for b, f in enumerate(items):
            if leaky and not np.isfinite(f[2]).all() and b + 1 < len(items):
                res[b + 1][0][6] = np.nextafter(res[b + 1][0][6], 1.0)          # one ulp in the neighbour's t_z
        return res
    empty = (odd[0], odd[1][:0], odd[2][:0], odd[3])
    without = batch([frames[0], empty, frames[1], frames[2]], False)
    check_neighbours(batch([frames[0], odd, frames[1], frames[2]], False), without, 1)
    with pytest.raises(AssertionError):
        check_neighbours(batch([frames[0], odd, frames[1], frames[2]], True), without, 1)
    ref = oracle.pose_only_optimize(*odd)
    check_classwise(odd[0], ref, ref)
    moved = (ref[0].copy(), ref[1], ref[2]); moved[0][4] = 1e-300
    with pytest.raises(AssertionError):
        check_classwise(odd[0], moved, ref)
    with pytest.raises(AssertionError):
        check_classwise(odd[0], (ref[0], ~ref[1], ref[2]), ref)
