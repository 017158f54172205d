"""Loop correction for a batch of maps (myslam_loop_correct_batch): the item builder shared by the CPU and GPU tests, the reference composition of
one item out of the one-map calls, in the reference's order (src/loopclosing.cpp:284-289, :328-330, :437-463), and the packing of items into the
strided device tables of include/myslam_hip.h with sentinels in every slot beyond a count.

An item starts from synth.pose_graph(n, loops, seed): its last loop edge (current key-frame -> loop key-frame) is dropped, because the call appends
it; the active window is the last n_active rows, cur the last row; the window is displaced by a right-multiplied rigid motion, so that fusion has work
to do and the need-correct gate |log(Tcur Tcc^-1)| is decided by that motion; the corrected pose is the dropped edge's measurement times the loop
key-frame's pose."""
import numpy as np

DONE, NOT_NEEDED, SKIPPED, FUSED_ONLY = 0, 1, 2, 3
ERR_INVALID, ERR_CAPACITY = -1, -3
MAX_SEPARATORS = 32
NEEDED_MOTION = np.array([1.5, -0.4, 0.8, 0.002, -0.003, 0.002])         # gate ~1.75: well above the threshold 1.0
SMALL_MOTION = np.array([0.3, -0.1, 0.2, 0.0005, -0.001, 0.0005])        # gate ~0.4: well below it
SENTINEL_F = -7.25e77
SENTINEL_I = -123456


def build_item(synth, oracle, n, loops, seed, n_active=10, needed=True, n_points=200, verify_status=0):
    poses, _, e0, e1, meas, gt = synth.pose_graph(n, loops, seed=seed, n_active=n_active)
    na = min(n_active, n - 1) if n > 1 else 1
    active = np.arange(n - na, n, dtype=np.int32)
    cur = n - 1
    rng = np.random.default_rng(seed + 1000)
    if len(e0) and e0[-1] == cur and e1[-1] < cur - 1:                    # synth's loop being closed
        loop = int(e1[-1]); m_loop = meas[-1].copy()
        e0, e1, meas = e0[:-1], e1[:-1], meas[:-1]
    else:                                                                 # too short a drive for synth to close a loop: close one onto key-frame 0
        loop = 0
        m_loop = oracle.se3_compose(oracle.se3_compose(gt[cur], gt[0], invert_b=True), oracle.se3_exp(0.003 * rng.standard_normal(6)))
    corrected = oracle.se3_compose(m_loop, poses[loop])
    poses = poses.copy()
    motion = oracle.se3_exp(NEEDED_MOTION if needed else SMALL_MOTION)
    for a in active:
        poses[a] = oracle.se3_compose(poses[a], motion)
    first_active = np.where(rng.uniform(size=n_points) < 0.4, rng.integers(0, na, n_points), -1).astype(np.int32)
    first_kf = rng.integers(-1, n, n_points).astype(np.int32)
    first_kf = np.where(first_active >= 0, active[np.maximum(first_active, 0)], first_kf).astype(np.int32)
    points = rng.normal(0, 30, (n_points, 3))
    return dict(n=n, poses=poses, active=active, cur=cur, loop=loop, corrected=corrected, e0=e0.astype(np.int32).copy(), e1=e1.astype(np.int32).copy(),
                meas=meas.copy(), points=points, first_active=first_active, first_kf=first_kf, verify_status=verify_status, gt=gt)


def fixed_of(item):
    fx = np.zeros(item["n"], np.uint8)
    fx[item["active"]] = 1; fx[item["loop"]] = 1; fx[0] = 1
    return fx


def add_short_loops(oracle, item, count, back=4, step=3, seed=5):
    """`count` extra loop edges (i, i - back) between FREE key-frames with distinct later endpoints i: one separator each"""
    rng = np.random.default_rng(seed)
    fx = fixed_of(item).astype(bool)
    cand = [i for i in range(back + 1, item["n"]) if not fx[i] and not fx[i - back]][::step][:count]
    assert len(cand) == count, (len(cand), count)
    gt = item["gt"]
    ms = [oracle.se3_compose(oracle.se3_compose(gt[i], gt[i - back], invert_b=True), oracle.se3_exp(0.003 * rng.standard_normal(6))) for i in cand]
    out = dict(item)
    out["e0"] = np.r_[item["e0"], np.array(cand, np.int32)].astype(np.int32)
    out["e1"] = np.r_[item["e1"], np.array(cand, np.int32) - back].astype(np.int32)
    out["meas"] = np.concatenate([item["meas"], np.array(ms).reshape(-1, 7)])
    return out


def gate_value(oracle, item):
    return float(np.linalg.norm(oracle.se3_log(oracle.se3_compose(item["poses"][item["cur"]], item["corrected"], invert_b=True))))


def reference(backend, oracle, item, threshold=1.0, iters=20):
    """The one-map calls in the reference's order.  `backend` supplies loop_local_fusion / pose_graph_optimize / correct_map_points (the oracle, or
    the library's host-pointer calls); the SE3 products of the edge and the gate always go through the oracle."""
    out = dict(status=SKIPPED, poses=item["poses"].copy(), points=item["points"].copy(), e0=item["e0"].copy(), e1=item["e1"].copy(),
               meas=item["meas"].copy(), chi2=0.0, iters=0)
    if item["verify_status"] != 0:
        return out
    out["e0"] = np.r_[item["e0"], item["cur"]].astype(np.int32); out["e1"] = np.r_[item["e1"], item["loop"]].astype(np.int32)
    out["meas"] = np.concatenate([item["meas"], oracle.se3_compose(item["corrected"], item["poses"][item["loop"]], invert_b=True)[None]])
    if gate_value(oracle, item) <= threshold:
        out["status"] = NOT_NEEDED
        return out
    active = item["active"]
    fa, pts = backend.loop_local_fusion(item["poses"][active], int(np.where(active == item["cur"])[0][0]), item["corrected"], item["first_active"], item["points"])
    fused = item["poses"].copy(); fused[active] = fa
    out["fused_poses"], out["fused_points"] = fused, pts
    opt, chi2, its = backend.pose_graph_optimize(fused, fixed_of(item), out["e0"], out["e1"], out["meas"], iters=iters)
    kf = np.where(item["first_active"] < 0, item["first_kf"], -1).astype(np.int32)
    out.update(status=DONE, poses=opt, points=backend.correct_map_points(fused, opt, kf, pts), chi2=chi2, iters=its)
    return out


def pack(items, kf_cap, edge_cap, active_cap, point_cap):
    """items -> the call's tables as numpy arrays, SENTINEL_F / SENTINEL_I in every slot beyond an item's count"""
    B = len(items)
    t = dict(poses=np.full((B, kf_cap, 7), SENTINEL_F), n_kf=np.zeros(B, np.int32), active=np.full((B, active_cap), SENTINEL_I, np.int32),
             n_active=np.zeros(B, np.int32), cur=np.zeros(B, np.int32), loop=np.zeros(B, np.int32), corrected=np.zeros((B, 7)),
             verify_status=np.zeros(B, np.int32), e0=np.full((B, edge_cap), SENTINEL_I, np.int32), e1=np.full((B, edge_cap), SENTINEL_I, np.int32),
             meas=np.full((B, edge_cap, 7), SENTINEL_F), n_edges=np.zeros(B, np.int32), points=np.full((B, point_cap, 3), SENTINEL_F),
             n_points=np.zeros(B, np.int32), first_active=np.full((B, point_cap), SENTINEL_I, np.int32), first_kf=np.full((B, point_cap), SENTINEL_I, np.int32))
    for b, it in enumerate(items):
        n, na, E, npt = it["n"], len(it["active"]), len(it["e0"]), len(it["points"])
        assert n <= kf_cap and na <= active_cap and E <= edge_cap and npt <= point_cap
        t["poses"][b, :n] = it["poses"]; t["n_kf"][b] = n; t["active"][b, :na] = it["active"]; t["n_active"][b] = na
        t["cur"][b] = it["cur"]; t["loop"][b] = it["loop"]; t["corrected"][b] = it["corrected"]; t["verify_status"][b] = it["verify_status"]
        t["e0"][b, :E] = it["e0"]; t["e1"][b, :E] = it["e1"]; t["meas"][b, :E] = it["meas"]; t["n_edges"][b] = E
        t["points"][b, :npt] = it["points"]; t["n_points"][b] = npt; t["first_active"][b, :npt] = it["first_active"]; t["first_kf"][b, :npt] = it["first_kf"]
    return t


IN_OUT = ("poses", "e0", "e1", "meas", "n_edges", "points")                # the tables the call may write
