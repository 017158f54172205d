"""The three pose solvers (k_ba_optimize, k_pose_only, PnP-RANSAC) on rigidly moved problems and on bad matches: world-frame
rotations that drive the three trace <= 0 branches of every R -> quaternion write-back, maps kilometres from the origin, negated and 3.7-fold
input quaternions, NaN / inf / 1e200 / behind-the-camera matches, and the count rule of myslam_pose_only_optimize_batch.

Every (problem, move) pair comes from tests/pose_cases.py and was qualified on the oracle alone by tests/test_pose_cases.py.  Two comparisons per
pair, both after move_back so that no tolerance grows with the kilometres:
  * against the oracle on the SAME moved inputs at the bars of test_gpu_ba.py / test_gpu_pose_only.py / test_gpu_pnp.py;
  * metamorphic: |move_back(GPU(moved)) - GPU(unmoved)| <= max(1e-9, 10 x d_ref), d_ref = the oracle's own distance for the pair (its sensitivity
    to the move; 10 for the other summation order).  This one never passes through the oracle's copy of the four-branch formula.
Pose-only at the table's own kilometre translations is judged by the far rule (check_po): there the oracle itself scatters by 2e-9 .. 5e-8 under
one-ulp changes of its inputs, so those five pairs are held to 10 x that scatter, and the same rotations run at 500 m under the full bars.
Measured on an MI355X: largest metamorphic distance 0.053 of its bar for BA, 0.087 pose-only, 0.100 PnP, 0.030 far pairs.
The checkers are plain functions of results: tests/test_pose_cases.py rehearses them on the CPU against faulty stand-ins."""
import numpy as np
import pytest

import pose_cases as PC

pytestmark = pytest.mark.gpu


# ---- checkers ---------------------------------------------------------------------------------------------------------------------
def _unit(q, tag):
    assert abs(np.sqrt(np.dot(q[:4], q[:4])) - 1.0) < 1e-12, (tag, "the quaternion written back is not a unit one", q[:4])


def _stat(tag, claim, pose, meta, d_ref):
    bar = max(1e-9, 10 * d_ref)
    assert meta <= bar, (tag, "metamorphic distance", meta, "bar", bar)
    return dict(tag=tag, claim=claim, branch=PC.branch_of(PC.R_of_q(pose[:4]))[0], wneg=bool(pose[3] < 0), meta=meta, d_ref=d_ref, ratio=meta / bar)


def check_po(r, got, base_got, tag="", claim=None, far=None):
    """one pose-only result (pose7, flags, inliers) on r["args"] against r["ref"], and against the same solver's result on the unmoved frame.
    far: the oracle's own scatter at kilometre offsets (Refs.far_scatter) for a pair of PO_FAR — flags, count, unit quaternion and branch as for
    every pair, the pose within 10 x that scatter of the oracle's and of the unmoved answer instead of the bars of test_gpu_pose_only.py."""
    pose, out, ni = got
    rp, rout, rni = r["ref"]
    _unit(pose, tag)
    assert int(ni) == rni and np.array_equal(np.asarray(out, bool), rout), (tag, "flags / inlier count", int(ni), rni)
    g, w = PC.move_back(r["G"], pose), PC.move_back(r["G"], rp)
    if far is None:
        assert np.allclose(PC.sign_align(g, w), w, rtol=1e-8, atol=1e-9), (tag, g, w)
    else:
        assert PC.pose_dist(g, w) <= max(1e-9, 10 * far), (tag, PC.pose_dist(g, w), far)
    return _stat(tag, claim, pose, PC.pose_dist(g, PC.canon(base_got[0])), r["d_ref"] if far is None else max(r["d_ref"], far))


def check_ba(r, got, base_got, tag="", claim=None):
    """one active-map result (poses, points, chi2, flags, rounds, outliers) on r["args"] against r["ref"] and the solver's unmoved result"""
    gp, gx, gchi, gout, gr, gn = got
    rp, rx, rchi, rout, rr, rn = r["ref"]
    for p in gp:
        _unit(p, tag)
    assert (int(gr), int(gn)) == (rr, rn), (tag, "rounds / outliers", gr, gn, rr, rn)
    far = ~(np.abs(rchi - PC.CHI2) < 1e-6)
    assert np.array_equal(np.asarray(gout)[far], rout[far]), (tag, "flags")
    assert np.allclose(gchi, rchi, rtol=1e-6, atol=1e-9), (tag, "chi2")
    bp, bx = PC.ba_back(r["G"], got)
    wp, wx = PC.ba_back(r["G"], r["ref"])
    for a, b in zip(bp, wp):
        assert np.allclose(PC.sign_align(a, b), b, rtol=1e-7, atol=1e-8), (tag, a, b)
    assert np.allclose(bx, wx, rtol=1e-7, atol=1e-7), (tag, "points", np.abs(bx - wx).max())
    fixed = r["args"][5].astype(bool)
    assert np.array_equal(gx[fixed], r["args"][1][fixed]), (tag, "a fixed landmark moved")
    meta = PC.ba_dist(r["G"], got, PC.IDENTITY, base_got)
    return [_stat(tag, claim, p, meta, r["d_ref"]) for p in gp]


def check_pnp(r, got, base_got, tag="", claim=None, strong=True):
    """one PnP result (pose7, mask, count) on r["args"] against r["ref"]; strong: the pose at 1e-9 against the oracle"""
    pose, inl, ni = got
    rc, rp, rin, rn = r["ref"]
    assert rc == 0, tag
    _unit(pose, tag)
    assert int(ni) == rn and np.array_equal(np.asarray(inl, bool), rin), (tag, "mask / count", int(ni), rn)
    g, w = PC.move_back(r["G"], pose), PC.move_back(r["G"], rp)
    if strong:
        assert PC.pose_dist(g, w) < 1e-9, (tag, g, w)
    return _stat(tag, claim, pose, PC.pose_dist(g, PC.canon(base_got[0])), r["d_ref"])


def check_seen(stats, solver):
    """from the solver's OWN outputs: every claiming pair took its branch, branches 1, 2 and 3 and a raw w < 0 were all seen"""
    for s in stats:
        assert s["claim"] is None or s["branch"] == s["claim"], (solver, s)
    seen = {s["branch"] for s in stats if s["claim"] is not None}
    assert {1, 2, 3} <= seen and any(s["wneg"] for s in stats), (solver, seen)
    worst = max(stats, key=lambda s: s["ratio"])
    print(f"{solver}: {len(stats)} poses, branches {sorted(seen)}, {sum(s['wneg'] for s in stats)} with raw w < 0; largest metamorphic distance / bar "
          f"{worst['ratio']:.3f} ({worst['tag']}: {worst['meta']:.1e}, d_ref {worst['d_ref']:.1e})")


def check_neighbours(with_odd, without_odd, odd, tag=""):
    """two runs of one batch that differ in item `odd` only (lists of per-item tuples of arrays / ints): every other item has the same bits"""
    assert len(with_odd) == len(without_odd)
    for b, (x, y) in enumerate(zip(with_odd, without_odd)):
        if b != odd:
            for u, v in zip(x, y):
                assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), (tag, "item", b, "changed beside the odd item", odd)


def check_classwise(T0, got, ref, tag=""):
    """a frame with a non-finite / overflowing match: the pose bytes unchanged where the oracle's are, flags and count the oracle's"""
    pose, out, ni = got
    rp, rout, rni = ref
    if rp.tobytes() == np.asarray(T0, np.float64).tobytes():
        assert pose.tobytes() == rp.tobytes(), (tag, "the oracle leaves the pose alone", pose)
    elif np.isfinite(rp).all():
        assert np.allclose(pose, rp, rtol=1e-8, atol=1e-9), (tag, pose, rp)
    else:
        assert np.array_equal(np.isfinite(pose), np.isfinite(rp)), (tag, pose, rp)
    assert int(ni) == rni and np.array_equal(np.asarray(out, bool), rout), (tag, "flags / count", int(ni), rni)


# ---- device runners -----------------------------------------------------------------------------------------------------------------
def po_batch(api, frames, cap, Kt, counts=None, spare=0, prefill=0):
    """frames: (T0, pts, obs) each -> [(pose7, flags[:n] as stored, inliers, status)]; `spare` more rows of cap behind every array"""
    import torch
    B = len(frames)
    poses = np.zeros((B + spare, 7)); poses[:, 3] = 1.0
    pts = np.zeros((B + spare, cap, 3)); obs = np.zeros((B + spare, cap, 2)); cnt = np.zeros(B + spare, np.int32)
    for b, (T0, p, o) in enumerate(frames):
        n = len(p); poses[b] = T0; pts[b, :n] = p; obs[b, :n] = o; cnt[b] = n
    if counts is not None:
        cnt[:B] = counts
    d = [torch.from_numpy(x).cuda() for x in (poses, pts, obs, cnt)]
    out = torch.full((B + spare, cap), prefill, dtype=torch.uint8, device="cuda")
    ni = torch.full((B + spare,), -7, dtype=torch.int32, device="cuda"); st = torch.full((B + spare,), -7, dtype=torch.int32, device="cuda")
    api.pose_only_optimize_batch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, cap, Kt, PC.CHI2, 4, 10,
                                 out.data_ptr(), ni.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    P, O, N, S = d[0].cpu().numpy(), out.cpu().numpy(), ni.cpu().numpy(), st.cpu().numpy()
    return [(P[b], O[b], int(N[b]), int(S[b])) for b in range(B + spare)]


def ba_batch(api, probs, maxP=7, maxL=120, maxE=900):
    """windows (poses, pts, ep, el, obs, fixed, K) -> [(poses, points, chi2, flags, rounds, outliers)] of one myslam_ba_optimize_active_map_batch"""
    import torch
    W = len(probs)
    poses = np.zeros((W, maxP, 7)); poses[..., 3] = 1
    pts = np.zeros((W, maxL, 3)); ep = np.zeros((W, maxE), np.int32); el = np.zeros((W, maxE), np.int32)
    obs = np.zeros((W, maxE, 2)); fixed = np.zeros((W, maxL), np.uint8); sizes = np.zeros((W, 3), np.int32)
    for w, (p, x, a, b, o, f, K) in enumerate(probs):
        assert len(p) <= maxP and len(x) <= maxL and len(a) <= maxE
        poses[w, :len(p)] = p; pts[w, :len(x)] = x; ep[w, :len(a)] = a; el[w, :len(a)] = b; obs[w, :len(a)] = o; fixed[w, :len(f)] = f
        sizes[w] = (len(p), len(x), len(a))
    d = [torch.from_numpy(a).cuda() for a in (poses, pts, ep, el, obs, fixed, sizes)]
    scratch = torch.zeros(W * maxE * 18, dtype=torch.float64, device="cuda")
    chi = torch.zeros(W, maxE, dtype=torch.float64, device="cuda"); out = torch.zeros(W, maxE, dtype=torch.uint8, device="cuda")
    rd = torch.zeros(W, dtype=torch.int32, device="cuda"); no = torch.zeros(W, dtype=torch.int32, device="cuda"); st = torch.ones(W, dtype=torch.int32, device="cuda")
    api.ba_optimize_active_map_batch(*[t.data_ptr() for t in d], W, maxP, maxL, maxE, probs[0][6], PC.CHI2, PC.CHI2, 5, 10, scratch.data_ptr(),
                                     chi.data_ptr(), out.data_ptr(), rd.data_ptr(), no.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    res = []
    for w, (p, x, a, b, o, f, K) in enumerate(probs):
        res.append((d[0][w, :len(p)].cpu().numpy(), d[1][w, :len(x)].cpu().numpy(), chi[w, :len(a)].cpu().numpy(), out[w, :len(a)].cpu().numpy(),
                    int(rd[w]), int(no[w])))
    return res


def nt_of(batch, cap):
    """pose_only_launch's table (csrc/ba.hip): threads per frame"""
    if batch >= 64:
        return 64 if cap <= 256 else (128 if cap <= 1024 else (256 if cap <= 2048 else 512))
    return 128 if cap <= 128 else (256 if cap <= 2048 else 512)


@pytest.fixture(scope="module")
def R(synth, oracle):
    return PC.refs(synth, oracle)


@pytest.fixture(scope="module")
def gpu_base(api, R):
    """the device's own answers on the unmoved problems (one-item calls), computed once"""
    cache = {}

    def get(kind, key):
        if (kind, key) not in cache:
            if kind == "po":
                cache[kind, key] = api.pose_only_optimize(*R.po(key, None, 1.0)["args"])
            elif kind == "ba":
                cache[kind, key] = api.ba_optimize_active_map(*R.ba(key, None, 1.0)["args"])
            else:
                cache[kind, key] = api.solve_pnp_ransac(*R.pnp(key, None, None)["args"])
        return cache[kind, key]
    return get


# ---- BA ---------------------------------------------------------------------------------------------------------------------------
def test_ba_moved_windows(api, oracle, R, gpu_base):
    """api.ba_optimize_active_map in the LDS form, the same window with the per-landmark state in HBM (bit-identical, as
    test_landmark_state_option_is_bit_identical demands), and api.ba_optimize (one optimize(10)) on every qualified pair"""
    stats = []
    for key, name, scale, claim in PC.BA_PAIRS:
        r = R.ba(key, name, scale)
        tag = f"ba {key} {name} x{scale}"
        a = api.ba_optimize_active_map(*r["args"])
        api.ba_set_option(api.BA_OPT_LANDMARKS_IN_HBM, 1)
        try:
            b = api.ba_optimize_active_map(*r["args"])
        finally:
            api.ba_set_option(api.BA_OPT_LANDMARKS_IN_HBM, 0)
        for x, y in zip(a[:4], b[:4]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), tag
        assert a[4:] == b[4:], tag
        s = check_ba(r, a, gpu_base("ba", key), tag, claim)
        print(f"{tag}: metamorphic {s[0]['meta']:.2e}, d_ref {s[0]['d_ref']:.2e}, of the bar {s[0]['ratio']:.3f}")
        stats += s
        gp, gx, gchi, git = api.ba_optimize(*r["args"], iters=10)
        rp, rx, rchi, rit = oracle.ba_optimize(*r["args"], iters=10)
        assert git == rit and gchi == pytest.approx(rchi, rel=1e-8), tag
        for p, q in zip(PC.ba_back(r["G"], (gp, gx))[0], PC.ba_back(r["G"], (rp, rx))[0]):
            assert np.allclose(PC.sign_align(p, q), q, rtol=1e-7, atol=1e-8), tag
        assert np.allclose(PC.points_back(r["G"], gx), PC.points_back(r["G"], rx), rtol=1e-7, atol=1e-7), tag
    check_seen(stats, "BA")


def test_ba_moved_batch(api, R, gpu_base):
    """one myslam_ba_optimize_active_map_batch of three windows, each under a different move"""
    pairs = PC.BA_BATCH
    assert len({p[1] for p in pairs}) == 3 and all(p in PC.BA_PAIRS for p in pairs)
    rs = [R.ba(k, nm, sc) for k, nm, sc, _ in pairs]
    res = ba_batch(api, [r["args"] for r in rs])
    stats = []
    for (k, nm, sc, claim), r, g in zip(pairs, rs, res):
        stats += check_ba(r, g, gpu_base("ba", k), f"ba batch {k} {nm} x{sc}", claim)
    assert {s["branch"] for s in stats} >= {1, 2, 3}


@pytest.mark.parametrize("kind", PC.BA_ODD)
def test_ba_bad_observation(api, oracle, synth, kind):
    """a NaN and a 1e200 observation in a window: rounds, outlier count and flags are the oracle's, the poses are compared where the oracle's are
    finite; in a batch the windows beside it keep their bits"""
    args = PC.ba_odd(synth, kind)
    ref = oracle.ba_optimize_active_map(*args)
    got = api.ba_optimize_active_map(*args)
    assert got[4:] == ref[4:], (got[4:], ref[4:])
    far = ~(np.abs(ref[2] - PC.CHI2) < 1e-6)
    assert np.array_equal(got[3][far], ref[3][far])
    fin = np.isfinite(ref[0]).all(1)
    assert fin.any() and np.allclose(got[0][fin], ref[0][fin], rtol=1e-7, atol=1e-8)
    assert np.array_equal(np.isfinite(got[0]).all(1), fin)
    clean = PC.ba_problem(synth, PC.BA_ODD_BASE)
    beside = [PC.ba_problem(synth, PC.BA_PROBLEMS["s"]), PC.ba_problem(synth, PC.BA_PROBLEMS["g"])]
    with_odd = ba_batch(api, [beside[0], args, beside[1]])
    without = ba_batch(api, [beside[0], clean, beside[1]])
    check_neighbours(with_odd, without, 1, kind)
    assert with_odd[1][4:] == ref[4:] and np.array_equal(with_odd[1][3][far], ref[3][far])


# ---- pose-only ----------------------------------------------------------------------------------------------------------------------
def test_pose_only_moved_one_frame(api, R, gpu_base):
    stats = []
    far = R.far_scatter()
    print(f"the oracle's own scatter at kilometre offsets: {far:.2e}")
    for key, name, scale, claim in PC.PO_PAIRS + PC.PO_BIG + PC.PO_FAR:
        r = R.po(key, name, scale)
        tag = f"pose-only {key} {name} x{scale}"
        is_far = (key, name, scale, claim) in PC.PO_FAR
        got = api.pose_only_optimize(*r["args"])
        s = check_po(r, got, gpu_base("po", key), tag, claim, far if is_far else None)
        print(f"{tag}: from the oracle {PC.pose_dist(PC.move_back(r['G'], got[0]), PC.move_back(r['G'], r['ref'][0])):.2e}, metamorphic {s['meta']:.2e}, "
              f"d_ref {s['d_ref']:.2e}, of the bar {s['ratio']:.3f}")
        stats.append(s)
    check_seen([s for s, p in zip(stats, PC.PO_PAIRS + PC.PO_BIG)], "pose-only, strong pairs")
    check_seen(stats[-len(PC.PO_FAR):], "pose-only, far pairs")


@pytest.mark.parametrize("batch,cap,nt", [(72, 200, 64), (72, 300, 128), (40, 300, 256), (40, 2105, 512)])
def test_pose_only_moved_block_sizes(api, R, batch, cap, nt):
    """every block size of pose_only_launch's table on differently moved frames in one batch; the unmoved frames ride in the same batch, so the
    metamorphic check compares results of the same block size; the same frame at two slots gives the same bits"""
    assert nt_of(batch, cap) == nt
    pairs = PC.PO_PAIRS + PC.PO_FAR + (PC.PO_BIG if cap > 2048 else [])
    far = R.far_scatter()
    items = [(k, nm, sc, cl) for k, nm, sc, cl in pairs] + [(k, None, 1.0, None) for k in dict.fromkeys(p[0] for p in pairs)]
    rs = [R.po(k, nm, sc) for k, nm, sc, _ in items]
    slots = [i % len(items) for i in range(batch)]
    assert batch > len(items) and all(len(r["args"][1]) <= cap for r in rs)
    res = po_batch(api, [rs[i]["args"][:3] for i in slots], cap, rs[0]["args"][3])
    assert all(x[3] == 0 for x in res)
    base_slot = {items[i][0]: i for i in range(len(items)) if items[i][1] is None}
    stats = []
    for b, i in enumerate(slots):
        k, nm, sc, claim = items[i]
        n = len(rs[i]["args"][1])
        got = (res[b][0], res[b][1][:n], res[b][2])
        assert not res[b][1][n:].any()                                 # slots from the count on are not written
        stats.append(check_po(rs[i], got, res[base_slot[k]], f"pose-only NT {nt} slot {b} {k} {nm} x{sc}", claim, far if items[i] in PC.PO_FAR else None))
        if b >= len(items):
            assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(res[b], res[i])), (b, i)
    check_seen([s for s, i in zip(stats, slots) if items[i] not in PC.PO_FAR], f"pose-only, {nt} threads per frame, strong pairs")
    check_seen([s for s, i in zip(stats, slots) if items[i] in PC.PO_FAR], f"pose-only, {nt} threads per frame, far pairs")


@pytest.mark.parametrize("kind", PC.PO_ODD)
def test_pose_only_bad_matches(api, oracle, synth, kind):
    args = PC.po_odd(synth, oracle, kind)
    ref = oracle.pose_only_optimize(*args)
    got = api.pose_only_optimize(*args)
    if kind == "behind3":
        assert (args[1][:, 2] < 0).sum() == 3 and np.isfinite(args[1]).all()
        assert np.allclose(got[0], ref[0], rtol=1e-8, atol=1e-9) and got[2] == ref[2] and np.array_equal(got[1], ref[1])
    else:
        check_classwise(args[0], got, ref, kind)
    beside = [R_args[:3] for R_args in (PC.po_problem(synth, oracle, PC.PO_PROBLEMS[k]) for k in ("a", "b", "c"))]
    empty = (args[0], args[1][:0], args[2][:0])
    with_odd = po_batch(api, [beside[0], args[:3], beside[1], beside[2]], 128, args[3])
    without = po_batch(api, [beside[0], empty, beside[1], beside[2]], 128, args[3])
    check_neighbours(with_odd, without, 1, kind)
    n = len(args[1])
    inb = (with_odd[1][0], with_odd[1][1][:n], with_odd[1][2])
    if kind == "behind3":
        assert np.allclose(inb[0], ref[0], rtol=1e-8, atol=1e-9) and inb[2] == ref[2] and np.array_equal(inb[1].astype(bool), ref[1])
    else:
        check_classwise(args[0], inb, ref, kind + " in a batch")


def test_pose_only_batch_count_rule(api, oracle, synth):
    """myslam_pose_only_optimize_batch reads a count below 0 as 0 and one above cap as cap.  Three frames, cap 64, counts [-3, cap + 9, 40], flags
    pre-filled with 255, one spare row of cap behind every array (so that a count read as it stands spills into memory the test owns)."""
    cap = 64
    frames, counts, Kt = PC.count_rule_frames(synth, oracle, cap)
    T0 = frames[0][0]
    res = po_batch(api, frames, cap, Kt, counts=counts, spare=1, prefill=255)
    assert res[0][2] == 0 and res[0][3] == 0 and res[0][0].tobytes() == T0.tobytes() and (res[0][1] == 255).all()
    r1 = oracle.pose_only_optimize(*frames[1], Kt)
    assert res[1][3] == 0 and res[1][2] == r1[2] and np.array_equal(res[1][1], r1[1].astype(np.uint8)) and np.allclose(res[1][0], r1[0], rtol=1e-8, atol=1e-9)
    r2 = oracle.pose_only_optimize(frames[2][0], frames[2][1][:40], frames[2][2][:40], Kt)
    assert res[2][3] == 0 and res[2][2] == r2[2] and np.array_equal(res[2][1][:40], r2[1].astype(np.uint8)) and np.allclose(res[2][0], r2[0], rtol=1e-8, atol=1e-9)
    assert (res[2][1][40:] == 255).all()
    assert (res[3][1] == 255).all() and res[3][2] == -7 and res[3][3] == -7            # the spare row: nothing beyond the batch is touched


# ---- PnP ----------------------------------------------------------------------------------------------------------------------------
def weak_pose_rule(pw, uv, Kt, pose, other_pose, ref, tag):
    """few inliers, a huge threshold or f32 points kilometres out: the pose at 1e-9 against the library's other entry point on the same item, and
    against the oracle by cost: the f64 sum of squared reprojection errors over the oracle's mask within a relative 1e-6.  Returns the measured value."""
    rc, rp, rin, rn = ref
    assert PC.pose_dist(pose, other_pose) < 1e-9, (tag, pose, other_pose)
    c_g, c_r = PC.reproj_cost(pw, uv, Kt, pose, rin), PC.reproj_cost(pw, uv, Kt, rp, rin)
    rel = abs(c_g - c_r) / c_r
    print(f"{tag}: cost over the oracle's {rn} inliers {c_g:.9g} against {c_r:.9g}: relative {rel:.2e}")
    assert rel <= 1e-6, (tag, rel)
    return rel


def test_pnp_moved_one_item(api, R, gpu_base):
    stats = []
    for key, name, max_t, claim in PC.PNP_PAIRS:
        r = R.pnp(key, name, max_t)
        tag = f"pnp {key} {name} |tg| <= {max_t}"
        s = check_pnp(r, api.solve_pnp_ransac(*r["args"]), gpu_base("pnp", key), tag, claim)
        print(f"{tag}: metamorphic {s['meta']:.2e}, d_ref {s['d_ref']:.2e}, of the bar {s['ratio']:.3f}")
        stats.append(s)
    check_seen(stats, "PnP")


def test_pnp_moved_batch(api, oracle, R, gpu_base):
    """PnPSolver.solve_batch and verify_batch on differently moved items in one batch, the far item (7.5 km, weak rule) among them"""
    from test_gpu_pnp_batch import SENTINEL, _Bufs, _pack
    pairs = PC.PNP_PAIRS + [PC.PNP_FAR]
    rs = [R.pnp(k, nm, mt) for k, nm, mt, _ in pairs]
    Kt = rs[0]["args"][2]
    bufs = _Bufs(len(pairs)); bufs.K = Kt
    bufs.load(*_pack([r["args"][:2] for r in rs]))
    solver = api.PnPSolver(len(pairs), 200, 100)
    bufs.solve(solver)
    out = bufs.results()
    stats = []
    for b, ((k, nm, mt, claim), r) in enumerate(zip(pairs, rs)):
        n = len(r["args"][0])
        tag = f"pnp batch {k} {nm} |tg| <= {mt}"
        assert out["st"][b] == 0 and not out["flag"][b][n:].any(), tag
        far = (k, nm, mt, claim) == PC.PNP_FAR
        got = (out["pose"][b], out["flag"][b][:n], out["ninl"][b])
        stats.append(check_pnp(r, got, gpu_base("pnp", k), tag, claim, strong=not far))
        one = api.solve_pnp_ransac(*r["args"])
        assert PC.pose_dist(got[0], one[0]) < 1e-9 and one[2] == got[2], tag
        if far:
            weak_pose_rule(r["args"][0], r["args"][1], Kt, got[0], one[0], r["ref"], tag)
    check_seen(stats, "PnP, batch")
    # the chain: PnP, then OptimizeCurrentPose over all matches from PnP's pose (the qualified items only)
    bufs.clear(); bufs.verify(solver)
    out = bufs.results()
    for b, ((k, nm, mt, claim), r) in enumerate(zip(pairs, rs)):
        if (k, nm, mt) not in PC.PNP_CHAIN:
            continue
        n = len(r["args"][0])
        p, o, ni = R.chain(k, nm, mt)
        tag = f"verify {k} {nm}"
        assert out["st"][b] == api.VERIFY_CONFIRMED and out["ninl"][b] == ni and np.array_equal(out["flag"][b][:n].astype(bool), o), tag
        _unit(out["pose"][b], tag)
        g, w = PC.move_back(r["G"], out["pose"][b]), PC.move_back(r["G"], p)
        assert np.allclose(PC.sign_align(g, w), w, rtol=1e-8, atol=1e-9), (tag, g, w)
        assert not np.array_equal(out["pose"][b], SENTINEL)
