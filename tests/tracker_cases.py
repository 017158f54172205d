"""Hand-made states of the multi-stream tracker (include/myslam_hip.h, myslam_tracker_set_frame accepts any state) at tiny sizes, for the
cases one rendered drive never reaches: rotations beyond 120 degrees, kilometre translations, feature counts on the 256-feature rounds of the
compaction, crafted keep patterns, the decision thresholds, landmarks at or behind the camera centre.  No GPU here: a case is
{"name", "st" (a state in api.Tracker.get_frame()'s layout), "prev", "cur" (images), "K", "outliers" (features whose landmark was displaced on
purpose), "lost" (features built to be lost)}.  tests/test_tracker_cases.py proves on tests/tracker_ref.py alone that every case reaches its
path; tests/test_gpu_tracker_edges.py runs the device against the same reference.

A state is geometrically consistent unless a case says otherwise: Tcw = rel_motion * last_rel * T(ref_pose) is the pose rule 1 predicts, the
features sit at seeded pixels of a textured image, each has a depth of 4 - 40 m and its landmark is the back-projection through Tcw^-1 (f64) of
the pixel where the feature appears in the current image."""
import numpy as np

SIZES = [(120, 160), (118, 157), (117, 160)]          # rows x cols: plain; odd cols; rows % 4 != 0.  win 11, max_level 3: top level >= 15 x 20
MARGIN = 16
CHI2 = 5.991


def K_of(rows, cols):
    return (120.0, 118.0, (cols - 1) / 2.0, (rows - 1) / 2.0)


def quat(axis, deg):
    a = np.asarray(axis, float); a = a / np.sqrt((a * a).sum())
    h = np.radians(deg) / 2.0
    return np.concatenate([np.sin(h) * a, [np.cos(h)]])


def pose7(q, t):
    return np.concatenate([np.asarray(q, float), np.asarray(t, float)])


def small_motion(chain, deg=0.2, cm=2.0):
    return chain.T_of(pose7(quat((0.3, 1.0, -0.2), deg), np.array([0.6, -0.3, 0.74]) * cm / 100.0))


def images(synth, seed, rows, cols, shift=(0, 0)):
    """(previous, current): the current image is the previous one, or the crop of the same larger image moved by shift = (dx, dy) whole pixels:
    a feature at (x, y) then appears at (x - dx, y - dy)"""
    big = synth.random_image(seed, rows + 16, cols + 16, "texture")
    prev = np.ascontiguousarray(big[8:8 + rows, 8:8 + cols])
    cur = np.ascontiguousarray(big[8 + shift[1]:8 + shift[1] + rows, 8 + shift[0]:8 + shift[0] + cols])
    return prev, cur


def back_project(chain, K, Tcw, uv, depth):
    """world points (f64) that Tcw and K project onto the pixels uv at the given depths"""
    pc = np.stack([(uv[:, 0] - K[2]) / K[0] * depth, (uv[:, 1] - K[3]) / K[1] * depth, depth], 1)
    Twc = chain.T_inv(Tcw)
    return np.array([chain.mv(Twc[:3, :3], p) + Twc[:3, 3] for p in pc], float).reshape(-1, 3)


def predicted_Tcw(chain, st):
    return chain.mm(chain.mm(st["rel_motion"], st["last_rel"]), chain.T_of(st["ref_pose"]))


def make(chain, synth, name, rows=120, cols=160, n=48, seed=1, ref_pose=None, last_rel=None, rel_motion=None, shift=(0, 0), outliers=(),
         off_px=9.0, ref_frame_id=4, next_frame_id=10, kf_every=0, status=1):
    """n features, feature i on landmark i; `outliers`: features whose landmark is displaced so that it projects off_px beside the feature"""
    rng = np.random.default_rng(1000 + seed)
    K = K_of(rows, cols)
    prev, cur = images(synth, seed, rows, cols, shift)
    st = {"ref_pose": np.array(chain.IDENT if ref_pose is None else ref_pose, float),
          "last_rel": np.array(np.eye(4) if last_rel is None else last_rel, float),
          "rel_motion": np.array(np.eye(4) if rel_motion is None else rel_motion, float),
          "ref_frame_id": ref_frame_id, "next_frame_id": next_frame_id, "status": status, "kf_every": kf_every, "frozen": 0,
          "outlier_list": np.zeros(0, np.int32)}
    xy = np.stack([rng.uniform(MARGIN, cols - 1 - MARGIN, n), rng.uniform(MARGIN, rows - 1 - MARGIN, n)], 1).astype(np.float32)
    target = xy.astype(np.float64) - np.array(shift, float)          # where the feature is in the current image
    for i in outliers:
        target[i] += off_px * np.array([1.0, -0.5]) * (1 if i % 2 else -1)
    st["xy"], st["lm"] = xy, np.arange(n, dtype=np.int32)
    st["lm_pos"] = back_project(chain, K, predicted_Tcw(chain, st), target, rng.uniform(4.0, 40.0, n))
    st["lm_outlier"] = np.zeros(n, np.uint8)
    return {"name": name, "st": st, "prev": prev, "cur": cur, "K": K, "outliers": sorted(outliers), "lost": []}


def share_landmark(case, a, b):
    """feature b becomes a second observation of feature a's landmark at a's pixel"""
    st = case["st"]
    st["xy"][b] = st["xy"][a]; st["lm"][b] = st["lm"][a]
    if a in case["outliers"] and b not in case["outliers"]:
        case["outliers"] = sorted(case["outliers"] + [b])
    return case


# ---- SE3: every branch of R_to_q, the sign flip, non-unit and negated quaternions, kilometre translations ----
def se3_cases(chain, synth):
    lr = chain.T_of(pose7(quat((0.2, -1.0, 0.4), 1.0), (0.4, -0.1, 0.6)))          # last.rel: a degree and half a metre since the key-frame
    sm = small_motion(chain)
    spec = [("x180", quat((1, 0, 0), 180.0), (1.0e3, -2.5e3, 5.0e3), None, (0, 0)),
            ("y180_negated", -quat((0, 1, 0), 180.0), (-4.0e3, 1.2e3, 9.0e3), None, (2, -1)),
            ("z180_scaled", 3.7 * quat((0, 0, 1), 180.0), (7.5e3, 3.0e3, -1.0e3), None, (0, 0)),
            ("skew170", quat((0.6, -0.5, 0.62), 170.0), (2.0e3, 8.0e3, -6.0e3), sm, (0, 0)),
            ("skew170_reversed", 3.7 * quat((0.3, 0.8, -0.52), -170.0), (-1.0e4, 4.0e3, 2.0e3), sm, (-1, 2)),
            ("d120", quat((1, 1, 1), 120.0), (1.0e4, -1.0e4, 1.0e3), None, (0, 0)),
            ("plain20_negated", -quat((0.1, 0.9, 0.2), 20.0), (3.0e3, 1.0e3, -8.0e3), None, (1, 1))]
    return [make(chain, synth, nm, seed=10 + k, ref_pose=pose7(q, t), last_rel=lr, rel_motion=rm, shift=sh, outliers=(3, 17, 30))
            for k, (nm, q, t, rm, sh) in enumerate(spec)]


def branch_of(R):
    """(branch of chain.R_to_q that R takes, whether its raw w is negative so that the quaternion is flipped)"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        return 0, False
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1, R[2, 1] - R[1, 2] < 0
    if R[1, 1] > R[2, 2]:
        return 2, R[0, 2] - R[2, 0] < 0
    return 3, R[1, 0] - R[0, 1] < 0


# ---- counts on the rounds of 256 and crafted keep patterns ----
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024]
LOST_KINDS = ("outside", "nan", "no_landmark")


def _lose(st, i, kind):
    if kind == "outside":
        st["xy"][i, 0] = -40.0
    elif kind == "nan":
        st["xy"][i, 0] = np.nan
    else:
        st["lm"][i] = -1


def count_case(chain, synth, n, pattern="mixed", seed=0, rows=120, cols=160):
    """pattern "mixed": every seventh feature lost (the three kinds in turn: each round of 256 has lost and kept ones from n = 4 on);
    "all_lost"; "last_kept".  Each holds outlier-flagged landmarks (kept, no pose-only row) and a pair of features on one landmark."""
    c = make(chain, synth, f"n{n}_{pattern}", rows, cols, n=n, seed=40 + seed)
    st = c["st"]
    if n >= 8:
        share_landmark(c, 1, 2)                          # two rows of the pose-only problem on one landmark
    if n >= 4:
        a, b = [i for i in range(n - 2, -1, -1) if i % 7 != 3 and i > 2][:2] if n >= 8 else (n - 2, n - 4)
        share_landmark(c, a, b)                          # two kept features on one outlier-flagged landmark: no pose-only row for either
        st["lm_outlier"][st["lm"][a]] = 1
    for i in range(n):
        if i % 11 == 5:
            st["lm_outlier"][st["lm"][i]] = 1
    for i in range(n):
        lose = {"mixed": i % 7 == 3, "all_lost": True, "last_kept": i != n - 1}[pattern]
        if lose:
            _lose(st, i, LOST_KINDS[(i // 7 + i) % 3]); c["lost"].append(i)
    return c


# ---- the `frame id - ref frame id <= 2` rule at 2 and at 3 ----
def fresh_cases(chain, synth):
    out = []
    for d in (2, 3):
        c = make(chain, synth, f"fresh_{d}", n=56, seed=60 + d, outliers=(5, 21, 22, 40), ref_frame_id=7, next_frame_id=7 + d)
        share_landmark(c, 21, 23)                        # two outlier features on landmark 21: the list holds it twice
        out.append(c)
    return out


# ---- landmarks at or behind the camera centre (identity pose) ----
BAD_LANDMARKS = [("nan", (0.0, 0.0, 0.0)), ("inf", (1.0, 0.0, 0.0)), ("mirrored", (1.0, 1.0, -5.0)), ("overflow", (1e300, 0.0, 1.0))]


def nonfinite_case(chain, synth, seed=70, per_kind=3):
    """40 consistent features, then per_kind features on each bad landmark.  Those with a non-finite start point sit on good pixels (only the
    start point loses them); the mirrored ones sit where their landmark projects, so that LK has a finite start it can keep."""
    n0 = 40
    c = make(chain, synth, "nonfinite", n=n0 + per_kind * len(BAD_LANDMARKS), seed=seed)
    st, K = c["st"], c["K"]
    c["kinds"] = {}
    for k, (kind, p) in enumerate(BAD_LANDMARKS):
        for j in range(per_kind):
            i = n0 + k * per_kind + j
            pw = np.array(p, float)
            if kind == "mirrored":
                pw = pw * np.array([1.0 if j % 2 == 0 else -1.0, 1.0 if j < 2 else -1.0, 1.0])
                st["xy"][i] = np.array([K[0] * pw[0] / pw[2] + K[2], K[1] * pw[1] / pw[2] + K[3]], np.float32)
            st["lm_pos"][i] = pw
            c["kinds"][i] = kind
    return c


def bank_cases(chain, synth, S, lo, hi, seed=80, rows=120, cols=160):
    """S streams with lo .. hi features each, counts varying, stream 3 empty"""
    rng = np.random.default_rng(seed)
    ns = rng.integers(lo, hi + 1, S); ns[3] = 0; ns[0] = lo; ns[1] = hi
    return [make(chain, synth, f"bank{s}", rows, cols, n=int(ns[s]), seed=seed + s, outliers=(2, 9) if ns[s] > 30 else ()) for s in range(S)]


def layout_cases(chain, synth, name, S, rows, cols):
    """(S cases, the third image of each stream: the crop moves on by one more pixel, so the second step tracks a real shift from the stored copy)"""
    cases = [make(chain, synth, f"{name}{s}", rows, cols, n=44, seed=20 + s, shift=(1, -1) if s else (0, 0), outliers=(4, 9, 31)) for s in range(S)]
    third = [images(synth, 20 + s, rows, cols, (2, -1) if s else (0, 1))[1] for s in range(S)]
    return cases, third


def cap4096_cases(chain, synth):
    return [make(chain, synth, f"cap4096_{n}", n=n, seed=90 + k, outliers=(7, 100, 2999)) for k, n in enumerate((4096, 3000))]


def threshold_case(chain, synth):
    return make(chain, synth, "thresholds", n=60, seed=50, outliers=(1, 11, 33))


KF_IDS = [(6, 12), (6, 13), (6, 0), (6, -6), (6, -5), (1, 7), (0, 7)]          # (kf_every, frame id)


def beside_cases(chain, synth):
    """the ordinary streams that run beside the non-finite one"""
    return make(chain, synth, "beside_a", n=50, seed=71, outliers=(3, 4, 5)), make(chain, synth, "beside_b", n=33, seed=72, shift=(1, 1))


def abi_case(chain, synth):
    return make(chain, synth, "abi_pitch", 118, 157, n=44, seed=25, shift=(1, 0), outliers=(2, 8, 20))


def keep_pattern_cases(chain, synth):
    spec = [(257, "all_lost"), None, (513, "last_kept"), (256, "last_kept"), (64, "all_lost"), (300, "mixed")]
    return [count_case(chain, synth, x[0], x[1], seed=20 + k) if x else None for k, x in enumerate(spec)]
