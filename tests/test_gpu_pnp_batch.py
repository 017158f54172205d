"""Loop verification for a batch of candidates on the device (myslam_solve_pnp_ransac_batch, myslam_loop_verify_batch through api.PnPSolver)
against the oracle and against the library's own one-item calls.

Bars (those of tests/test_gpu_pnp.py and tests/test_gpu_pose_only.py): consensus mask, counts and status exact; PnP's pose to 1e-9 with the
quaternion sign aligned; the optimised pose to rtol 1e-8 / atol 1e-9, outlier flags and inlier count exact.  The 1e-9 bar on PnP's pose against the
ORACLE holds for items with at least 20 oracle inliers (the smallest count test_gpu_pnp.py holds it at); smaller items are weak problems whose
refinement amplifies the last bits of sin / cos, and their pose is held at 1e-9 against api.solve_pnp_ransac on the same item instead.

Every batch is at most 12 items of at most 200 points; the oracle's answers are computed once per problem and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 200
SENTINEL = np.array([0.5, -0.25, 0.125, 7.0, 11.0, -13.0, 17.0])
WEAK = (12, 7)        # (n, seed) of the item whose chain ends below 10 inliers: see test_verify_chain


def _noise_item():
    """the pure-noise item of tests/test_gpu_pnp.py:47-49: no model"""
    rng = np.random.default_rng(0)
    return rng.normal(0, 10, (80, 3)).astype(np.float32), rng.uniform(0, 1000, (80, 2)).astype(np.float32)


@pytest.fixture(scope="module")
def problems(synth, oracle, api):
    """item(n, seed) -> (pw, uv); K; cached answers of the oracle and of the library's one-item calls"""
    K = synth.pnp_problem(5, 0.3, 0.5, 11)[2]

    @functools.lru_cache(maxsize=None)
    def item(n, seed):
        if n == "noise":
            return _noise_item()
        if n == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
        pw, uv, Kt, _, _ = synth.pnp_problem(n, 0.3, 0.5, seed)
        assert Kt == K
        return pw, uv

    @functools.lru_cache(maxsize=None)
    def ref_pnp(n, seed, iterations=100, reproj_error=5.991, confidence=0.99):
        pw, uv = item(n, seed)
        if len(pw) == 0:
            return -4, None, np.zeros(0, bool), 0
        return oracle.solve_pnp_ransac(pw, uv, K, iterations=iterations, reproj_error=reproj_error, confidence=confidence)

    @functools.lru_cache(maxsize=None)
    def ref_chain(n, seed):
        """the oracle's two stages: PnP, then OptimizeCurrentPose over all matches from PnP's pose"""
        pw, uv = item(n, seed)
        rc, rp, rin, rn = ref_pnp(n, seed)
        if rc != 0:
            return None
        return oracle.pose_only_optimize(rp, pw.astype(np.float64), uv.astype(np.float64), K, pre_optimize=1)

    @functools.lru_cache(maxsize=None)
    def lib_pnp(n, seed, iterations=100, reproj_error=5.991, confidence=0.99):
        pw, uv = item(n, seed)
        try:
            return api.solve_pnp_ransac(pw, uv, K, iterations=iterations, reproj_error=reproj_error, confidence=confidence)
        except api.MyslamError as e:
            assert e.code == api.ERR_UNSUPPORTED
            return None

    @functools.lru_cache(maxsize=None)
    def lib_chain(n, seed):
        pw, uv = item(n, seed)
        g = lib_pnp(n, seed)
        if g is None:
            return None
        return api.pose_only_optimize(g[0], pw.astype(np.float64), uv.astype(np.float64), K, pre_optimize=1)

    class P:
        pass
    P.K, P.item, P.ref_pnp, P.ref_chain, P.lib_pnp, P.lib_chain = K, item, ref_pnp, ref_chain, lib_pnp, lib_chain
    return P


def _pack(items, cap=CAP, counts=None):
    """batch x cap arrays, every slot from an item's count on filled with NaN"""
    B = len(items)
    p3 = np.full((B, cap, 3), np.nan, np.float32); p2 = np.full((B, cap, 2), np.nan, np.float32); cnt = np.zeros(B, np.int32)
    for b, (pw, uv) in enumerate(items):
        n = len(pw); p3[b, :n] = pw; p2[b, :n] = uv; cnt[b] = n
    if counts is not None:
        cnt[:] = counts
    return p3, p2, cnt


class _Bufs:
    """device inputs and pre-filled outputs of one call: pose = a sentinel, flags 255, ints -7"""

    def __init__(self, B, cap=CAP):
        import torch
        self.torch, self.B, self.cap = torch, B, cap
        self.p3 = torch.zeros(B, cap, 3, dtype=torch.float32, device="cuda"); self.p2 = torch.zeros(B, cap, 2, dtype=torch.float32, device="cuda")
        self.cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.pose = torch.zeros(B, 7, dtype=torch.float64, device="cuda"); self.flag = torch.zeros(B, cap, dtype=torch.uint8, device="cuda")
        self.ninl = torch.zeros(B, dtype=torch.int32, device="cuda"); self.st = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.pnp_pose = torch.zeros(B, 7, dtype=torch.float64, device="cuda"); self.pnp_flag = torch.zeros(B, cap, dtype=torch.uint8, device="cuda")
        self.sentinel = torch.from_numpy(np.tile(SENTINEL, (B, 1))).cuda()

    def load(self, p3, p2, cnt):
        t = self.torch
        self.p3.copy_(t.from_numpy(p3)); self.p2.copy_(t.from_numpy(p2)); self.cnt.copy_(t.from_numpy(cnt))
        self.clear()

    def clear(self):
        self.pose.copy_(self.sentinel); self.pnp_pose.copy_(self.sentinel)
        self.flag.fill_(255); self.pnp_flag.fill_(255); self.ninl.fill_(-7); self.st.fill_(-7)

    def solve(self, solver, batch=None, **kw):
        solver.solve_batch(self.p3.data_ptr(), self.p2.data_ptr(), self.cnt.data_ptr(), batch or self.B, self.K, self.pose.data_ptr(), self.flag.data_ptr(),
                           self.ninl.data_ptr(), self.st.data_ptr(), **kw)

    def verify(self, solver, pnp_out=True, **kw):
        solver.verify_batch(self.p3.data_ptr(), self.p2.data_ptr(), self.cnt.data_ptr(), self.B, self.K, self.pose.data_ptr(), self.flag.data_ptr(),
                            self.ninl.data_ptr(), self.st.data_ptr(), self.pnp_pose.data_ptr() if pnp_out else 0,
                            self.pnp_flag.data_ptr() if pnp_out else 0, **kw)

    def results(self):
        self.torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("pose", "flag", "ninl", "st", "pnp_pose", "pnp_flag")}


def _pose_close(g, r, tol=1e-9):
    s = np.sign(np.dot(g[:4], r[:4]))
    return np.abs(g[:4] * s - r[:4]).max() < tol and np.abs(g[4:] - r[4:]).max() < tol


def _check_pnp_item(P, key, pose, flag, ninl, st, n_eff=None, **kw):
    """one item of a solve_batch result against the oracle (ints) and the oracle / the one-item call (pose); returns 'none' or whether the pose
    has the one-item call's bits"""
    pw, uv = P.item(*key)
    n = len(pw) if n_eff is None else n_eff
    rc, rp, rin, rn = P.ref_pnp(*key, **kw)
    assert (flag[n:] == 0).all(), key                       # slots from the count on are written as 0
    if rc != 0:                                             # no model: status 1, pose untouched, mask row zero
        assert st == 1 and ninl == 0 and (flag == 0).all() and np.array_equal(pose, SENTINEL), key
        assert n < 5 or P.lib_pnp(*key, **kw) is None, key
        return "none"
    assert st == 0 and ninl == rn and np.array_equal(flag[:n].astype(bool), rin), key
    gp, gin, gn = P.lib_pnp(*key, **kw)
    assert gn == rn and np.array_equal(gin, rin), key
    assert _pose_close(pose, gp), (key, pose, gp)
    if rn >= 20:
        assert _pose_close(pose, rp), (key, pose, rp)
    return np.array_equal(pose, gp)


def test_mixed_batch(api, problems):
    P = problems
    keys = [(n, 11) for n in (0, 4, 5, 9, 10, 12, 63, 64, 65, 128, 200)] + [("noise", 0)]
    bufs = _Bufs(len(keys)); bufs.K = P.K
    bufs.load(*_pack([P.item(*k) for k in keys]))
    solver = api.PnPSolver(len(keys), CAP, 100)
    bufs.solve(solver)
    r = bufs.results()
    verdicts = [_check_pnp_item(P, k, r["pose"][b], r["flag"][b], r["ninl"][b], r["st"][b]) for b, k in enumerate(keys)]
    none = [k for k, v in zip(keys, verdicts) if v == "none"]
    assert none == [(0, 11), (4, 11), (5, 11), ("noise", 0)], none          # only the four model-less items leave the pose comparison
    assert [int(x) for x in r["ninl"]] == [0, 0, 0, 6, 7, 8, 44, 45, 45, 90, 140, 0]
    same = [v for v in verdicts if v != "none"]
    print(f"mixed batch: {sum(same)} of {len(same)} poses carry the bits of api.solve_pnp_ransac on the same item")


def test_parameters_limits_and_counts(api, problems):
    P = problems
    solver = api.PnPSolver(2, CAP, 300)
    bufs = _Bufs(2); bufs.K = P.K
    key = (65, 11)
    bufs.load(*_pack([P.item(*key), P.item(*key)]))
    for iterations in (10, 300):
        kw = dict(iterations=iterations, reproj_error=2.0, confidence=0.999)
        bufs.clear(); bufs.solve(solver, batch=1, **kw)
        r = bufs.results()
        assert _check_pnp_item(P, key, r["pose"][0], r["flag"][0], r["ninl"][0], r["st"][0], **kw) != "none"
        assert r["st"][1] == -7 and np.array_equal(r["pose"][1], SENTINEL)                       # batch 1: item 1 is not touched
    bufs.clear()
    with pytest.raises(api.MyslamError) as e:
        bufs.solve(solver, batch=1, iterations=301)
    assert e.value.code == api.ERR_CAPACITY
    with pytest.raises(api.MyslamError) as e:
        bufs.solve(solver, batch=3)
    assert e.value.code == api.ERR_CAPACITY
    with pytest.raises(api.MyslamError) as e:
        bufs.verify(solver, iterations=301)
    assert e.value.code == api.ERR_CAPACITY
    r = bufs.results()
    assert (r["st"] == -7).all() and (r["flag"] == 255).all()                                     # refused before anything was enqueued
    # counts below 0 are 0, counts above cap are cap
    full = (200, 11)
    bufs.load(*_pack([P.item(0, 11), P.item(*full)], counts=[-3, CAP + 7]))
    bufs.solve(solver)
    r = bufs.results()
    assert _check_pnp_item(P, (0, 11), r["pose"][0], r["flag"][0], r["ninl"][0], r["st"][0]) == "none"
    assert _check_pnp_item(P, full, r["pose"][1], r["flag"][1], r["ninl"][1], r["st"][1]) != "none"
    with pytest.raises(api.MyslamError) as e:
        api.PnPSolver(1, 4097, 100)
    assert e.value.code == api.ERR_CAPACITY
    with pytest.raises(api.MyslamError) as e:
        api.PnPSolver(1, CAP, 100001)
    assert e.value.code == api.ERR_CAPACITY


def test_batch_of_one_and_reuse(api, problems):
    """the same handle on a large item, a small one and a model-less one: nothing of an earlier call's workspace shows"""
    P = problems
    solver = api.PnPSolver(1, CAP, 100)
    bufs = _Bufs(1); bufs.K = P.K
    for key in ((128, 12), (63, 12), (4, 12), (12, 12), (200, 12)):
        bufs.load(*_pack([P.item(*key)]))
        bufs.solve(solver)
        r = bufs.results()
        v = _check_pnp_item(P, key, r["pose"][0], r["flag"][0], r["ninl"][0], r["st"][0])
        assert (v == "none") == (key == (4, 12))


def _oracle_is_stable(P, oracle, key):
    """the method of tests/golden/make_pose_only_weak_frame.py: the oracle's second stage on eight seeded one-ulp perturbations of the observations"""
    pw, uv = P.item(*key)
    rp = P.ref_pnp(*key)[1]
    p, o, n = P.ref_chain(*key)
    rng = np.random.default_rng(0)
    obs = uv.astype(np.float64)
    for _ in range(8):
        q = oracle.pose_only_optimize(rp, pw.astype(np.float64), obs * (1 + rng.choice([-1.0, 1.0], size=obs.shape) * 2.2e-16), P.K, pre_optimize=1)
        if q[2] != n or not np.array_equal(q[1], o) or np.abs(q[0] - p).max() > 1e-12:
            return False
    return True


def _check_chain_item(P, api, key, r, b):
    pw, uv = P.item(*key)
    n = len(pw)
    pose, flag, ninl, st = r["pose"][b], r["flag"][b], int(r["ninl"][b]), int(r["st"][b])
    assert (flag[n:] == 0).all() and (r["pnp_flag"][b][n:] == 0).all(), key
    if n < 10:
        assert st == api.VERIFY_FEW_MATCHES and np.array_equal(pose, SENTINEL) and ninl == 0 and (flag == 0).all(), key
        assert np.array_equal(r["pnp_pose"][b], SENTINEL) and (r["pnp_flag"][b] == 0).all(), key
        return st
    ref, lib = P.ref_chain(*key), P.lib_chain(*key)
    if ref is None:
        assert lib is None and st == api.VERIFY_NO_MODEL and np.array_equal(pose, SENTINEL) and ninl == 0 and (flag == 0).all(), key
        assert np.array_equal(r["pnp_pose"][b], SENTINEL) and (r["pnp_flag"][b] == 0).all(), key
        return st
    # PnP's own outputs, as the lock-step checkers record them
    rc, rp, rin, rn = P.ref_pnp(*key)
    gp, gin, gn = P.lib_pnp(*key)
    assert np.array_equal(r["pnp_flag"][b][:n].astype(bool), rin) and _pose_close(r["pnp_pose"][b], gp), key
    # the chain against the oracle's two stages ...
    p, o, ni = ref
    s = np.sign(np.dot(pose[:4], p[:4])); aligned = np.concatenate([pose[:4] * s, pose[4:]])
    assert np.allclose(aligned, p, rtol=1e-8, atol=1e-9), (key, pose, p)
    assert ninl == ni and np.array_equal(flag[:n].astype(bool), o), key
    # ... and against the two one-item calls of the library
    lp, lo, lni = lib
    assert _pose_close(pose, lp) and ninl == lni and np.array_equal(flag[:n].astype(bool), lo), (key, pose, lp)
    assert st == (api.VERIFY_CONFIRMED if ni >= 10 else api.VERIFY_FEW_INLIERS), key
    return st


VERIFY_KEYS = [(63, 11), (64, 11), (65, 11), (128, 11), (200, 11), (9, 11), ("noise", 0), WEAK]


def test_verify_chain(api, oracle, problems):
    """ComputeCorrectPose's arithmetic in one enqueue.  The FEW_INLIERS item is synth.pnp_problem(12, 0.3, 0.5, seed=7): the oracle finds a model on
    8 of its 12 matches, its second stage keeps 8 (< 10), and eight one-ulp perturbations of the observations leave flags and count as they are and
    the pose within 1e-12 (seeds 0..49 at n = 12 were searched on the CPU; 26 of them are stable in this sense, 7 moves least: 5e-15)."""
    P = problems
    assert P.ref_chain(*WEAK)[2] < 10 and _oracle_is_stable(P, oracle, WEAK)
    bufs = _Bufs(len(VERIFY_KEYS)); bufs.K = P.K
    bufs.load(*_pack([P.item(*k) for k in VERIFY_KEYS]))
    solver = api.PnPSolver(len(VERIFY_KEYS), CAP, 100)
    bufs.verify(solver)
    r = bufs.results()
    st = [_check_chain_item(P, api, k, r, b) for b, k in enumerate(VERIFY_KEYS)]
    assert st == [api.VERIFY_CONFIRMED] * 5 + [api.VERIFY_FEW_MATCHES, api.VERIFY_NO_MODEL, api.VERIFY_FEW_INLIERS]
    assert [int(x) for x in r["ninl"]] == [44, 45, 45, 90, 140, 0, 0, 8]
    # PnP's pose and mask are optional
    bufs.clear(); bufs.verify(solver, pnp_out=False)
    r2 = bufs.results()
    assert all(np.array_equal(r[k], r2[k]) for k in ("pose", "flag", "ninl", "st"))
    assert (r2["pnp_flag"] == 255).all() and np.array_equal(r2["pnp_pose"], np.tile(SENTINEL, (len(VERIFY_KEYS), 1)))


def test_verify_recorded(api, problems):
    """verify_batch recorded once into a StepGraph (no side streams) and replayed on rewritten inputs: each replay has the eager call's bits"""
    import torch
    P = problems
    sets = [[(63, 11), (9, 11), (128, 11), WEAK], [("noise", 0), (200, 12), (12, 12), (65, 12)]]
    stream = torch.cuda.Stream()
    solver = api.PnPSolver(4, CAP, 100, stream=stream.cuda_stream)
    bufs = _Bufs(4); bufs.K = P.K
    eager = []
    with torch.cuda.stream(stream):
        for keys in sets:
            bufs.load(*_pack([P.item(*k) for k in keys]))
            bufs.verify(solver)
            eager.append(bufs.results())
        assert not all(np.array_equal(eager[0][k], eager[1][k]) for k in eager[0])
        g = api.StepGraph.record(stream.cuda_stream, [], lambda: bufs.verify(solver))
        assert g.node_count() >= 6           # sampling, hypotheses, select + refine, widening, pose-only, verdict
        for keys, want in zip(sets, eager):
            bufs.load(*_pack([P.item(*k) for k in keys]))
            g.launch(stream.cuda_stream)
            got = bufs.results()
            for k in want:
                assert np.array_equal(got[k], want[k]), k
