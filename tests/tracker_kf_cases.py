"""Hand-made streams for the key-frame turn of the multi-stream tracker (include/myslam_hip.h, myslam_tracker_keyframe_*) at the sizes of
tests/tracker_cases.py.  No GPU here.  A case is {"name", "st" (api.Tracker.set_frame's dict), "ids" (set_ids' arguments), "left" (the stored image),
"right" (the left image moved by d whole pixels: a feature at (x, y) is at (x - d, y) there, so the disparity is d), "new_xy" (the detected
key-points), "K", "d", "near" (features whose landmark projects far outside the right image)}.  tests/test_tracker_kf_ref.py proves on
tests/tracker_kf_ref.py and the oracle's operators that every case is made of what its name says; tests/test_gpu_tracker_kf.py runs the device."""
import numpy as np

import tracker_cases as TC

BASELINE = 0.5
DEPTH = 20.0                                       # fx * BASELINE / DEPTH = 3 px: the disparity of the plain cases
GOOD, BAD = 20, -1                                 # tracking_bad -1: a stepped stream is never LOST; kf_every 1 freezes it by the key-frame rule
TOTALS = [0, 1, 63, 64, 65, 255, 256, 257, 513, 1024]          # n_feat + n_new on the rounds of 256 of the turn's tail


def ids_of(n, base=100, stride=3):
    """landmark ids that are neither slots nor contiguous; counters above them"""
    lid = base + stride * np.arange(n, dtype=np.int64)
    return {"landmark_id": lid, "ref_kf_id": 7, "next_kf_id": 12, "next_mp_id": int(base + stride * n + 5)}


def new_points(rows, cols, n_new, seed):
    rng = np.random.default_rng(5000 + seed)
    return np.stack([rng.uniform(TC.MARGIN, cols - 1 - TC.MARGIN, n_new), rng.uniform(TC.MARGIN, rows - 1 - TC.MARGIN, n_new)], 1).astype(np.float32)


def make(chain, synth, name, rows=120, cols=160, n=48, n_new=16, seed=1, d=3, ref_pose=None, last_rel=None, no_lm=(), flagged=(), shared=(), near=()):
    """n features (feature i on landmark i at DEPTH in front of Tcw = last_rel * T(ref_pose)), n_new detected key-points.  no_lm: kept features
    without a landmark (their landmarks stay in the table, unreferenced); flagged: features whose landmark is marked outlier; shared: pairs
    (a, b), b becomes a second observation of a's landmark; near: features whose landmark is 0.25 m away (disparity 240 px: the right start
    point lies far outside the image)"""
    c = TC.make(chain, synth, name, rows, cols, n=n, seed=seed, ref_pose=ref_pose, last_rel=last_rel, kf_every=0)
    st, K = c["st"], c["K"]
    depth = np.full(n, DEPTH)
    depth[list(near)] = 0.25
    st["lm_pos"] = TC.back_project(chain, K, chain.mm(st["last_rel"], chain.T_of(st["ref_pose"])), st["xy"].astype(np.float64), depth)
    for a, b in shared:
        TC.share_landmark(c, a, b)
    for i in flagged:
        st["lm_outlier"][st["lm"][i]] = 1
    for i in no_lm:
        st["lm"][i] = -1
    return {"name": name, "st": st, "ids": ids_of(n), "left": c["prev"], "right": TC.images(synth, seed, rows, cols, (d, 0))[1], "K": K, "d": d,
            "new_xy": new_points(rows, cols, n_new, seed), "near": sorted(near)}


def rich_case(chain, synth, **kw):
    """everything at once: a kept feature without a landmark in the middle of the table (13, 14), a referenced landmark that is marked outlier (5;
    20 shares it), two features on one landmark (1 and 2), right tracks lost outside the image (30, 31)"""
    return make(chain, synth, "rich", n=48, n_new=16, seed=3, no_lm=(13, 14), flagged=(5,), shared=((1, 2), (5, 20)), near=(30, 31), **kw)


def total_case(chain, synth, total, seed=0):
    """n_feat + n_new = total, about two thirds kept; a shared landmark, a flagged one and a feature without a landmark from 8 features on"""
    n = (2 * total + 2) // 3
    kw = dict(no_lm=(3,), flagged=(4,), shared=((1, 2),)) if n >= 8 else {}
    return make(chain, synth, f"total{total}", n=n, n_new=total - n, seed=200 + seed, **kw)


def disparity_cases(chain, synth):
    """disparity 0 and -2: the right image is the left one / moved the wrong way, so no new point lies in front of the cameras"""
    return [make(chain, synth, f"disparity{d}", n=24, n_new=24, seed=210 + k, d=d) for k, d in enumerate((0, -2))]


def se3_cases(chain, synth):
    """the R_to_q branch poses of tracker_cases.se3_cases as reference poses of a turn (Tcw, Twc and the new key-frame's pose take each branch)"""
    out = []
    for k, c in enumerate(TC.se3_cases(chain, synth)):
        st = c["st"]
        out.append(make(chain, synth, "se3_" + c["name"], n=24, n_new=12, seed=220 + k, ref_pose=st["ref_pose"], last_rel=st["last_rel"], no_lm=(7,)))
    return out


def size_cases(chain, synth):
    return [make(chain, synth, f"size{r}x{c}", r, c, n=40, n_new=20, seed=230 + k, no_lm=(9,), shared=((1, 2),)) for k, (r, c) in enumerate(TC.SIZES)]


# ---- masks: hand-made coordinates (a table may hold anything: myslam_tracker_set_frame accepts any state) ----
def mask_tables(rows, cols, cap):
    """{name: xy}"""
    half = np.array([[50.5, 40.5], [51.5, 41.5], [20.5, 19.5], [21.5, 20.5]], np.float32)          # x - 20 = 30.5 -> 30 (even), 31.5 -> 32; 0.5 -> 0, 1.5 -> 2
    borders = np.array([[3.0, 60.0], [cols - 2.25, 30.0], [80.0, 1.75], [70.0, rows - 1.0], [0.0, 0.0], [cols - 1.0, rows - 1.0],
                        [-20.0, 50.0], [cols + 19.0, 50.0], [40.0, -20.5], [40.0, rows + 19.5]], np.float32)
    outside = np.array([[-21.0, 50.0], [cols + 20.0, 50.0], [60.0, -21.5], [60.0, rows + 20.5], [-500.0, -500.0], [1e9, 10.0], [-1e30, 1e30]], np.float32)
    overlap = np.array([[60.0, 60.0], [70.0, 65.0], [75.25, 58.5], [60.0, 60.0]], np.float32)
    nonfinite = np.array([[np.nan, 30.0], [30.0, np.inf], [-np.inf, np.nan], [100.0, 80.0]], np.float32)
    rng = np.random.default_rng(77)
    full = np.stack([rng.uniform(-30, cols + 30, cap), rng.uniform(-30, rows + 30, cap)], 1).astype(np.float32)
    return {"half": half, "borders": borders, "outside": outside, "overlap": overlap, "empty": np.zeros((0, 2), np.float32), "nonfinite": nonfinite,
            "full": full}


def table_state(chain, xy):
    """a state that holds the table xy and nothing else (no landmarks)"""
    n = len(xy)
    return {"xy": np.asarray(xy, np.float32).reshape(-1, 2), "lm": np.full(n, -1, np.int32), "lm_pos": np.zeros((0, 3)), "lm_outlier": np.zeros(0, np.uint8),
            "ref_pose": chain.IDENT.copy(), "ref_frame_id": 4, "last_rel": np.eye(4), "rel_motion": np.eye(4), "next_frame_id": 10, "status": 1, "kf_every": 0}
