"""The key-frame turn of the multi-stream tracker on the GPU (csrc/tracker.hip: myslam_tracker_keyframe_masks / _keyframe_batch /
_update_from_map_batch / _set_image_batch) against tests/tracker_kf_ref.py, the walk that tests/test_tracker_kf_ref.py pins to the chain.
Masks: whole arrays byte for byte.  Turn: the walk is fed the device's right tracks and the device's triangulation — themselves checked bit for bit
against myslam_lk_track and myslam_triangulate_stereo on the same images and points — and every output array and the whole post-state (get_frame,
get_ids, stored image) must be its bytes.  Hand-made streams of tests/tracker_kf_cases.py at 120 x 160, 118 x 157, 117 x 160."""
import numpy as np
import pytest

import tracker_cases as TC
import tracker_kf_cases as KC
import tracker_kf_ref as KR

pytestmark = pytest.mark.gpu

CAP, LM_CAP, KP_CAP = 1024, 2048, 400
B = KC.BASELINE
OUT_SPEC = {"new_kf_id": ((), "int64"), "new_kf_pose": ((7,), "float64"), "feat_mp_id": (("cap",), "int64"), "feat_mp_pos": (("cap", 3), "float64"),
            "feat_uv": (("cap", 2), "float32"), "feat_tag": (("cap",), "int32"), "feat_flags": (("cap",), "uint8"), "n_feat": ((), "int32"),
            "outlier_mp_id": (("cap2",), "int64"), "n_outlier_mp": ((), "int32"), "right_xy": (("cap", 2), "float32"), "right_ok": (("cap",), "uint8"),
            "report": ((8,), "int32")}
STATE_KEYS = ("xy", "lm", "lm_pos", "lm_outlier", "ref_pose", "ref_frame_id", "last_rel", "rel_motion", "next_frame_id", "status", "kf_every", "frozen",
              "outlier_list", "image")
_cache = {}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _state_bytes(st, ids):
    return [np.asarray(st[k]).tobytes() for k in STATE_KEYS] + [np.asarray(ids[k]).tobytes() for k in sorted(ids)]


class Rig:
    """a tracker of S streams with the device buffers of a turn; pitch > cols pads the rows of the right images and the masks; stride: bytes from
    one stream's image to the next (the default keeps every stream's base 4-byte aligned when the pitch is a multiple of 4)"""

    def __init__(self, api, S, rows=120, cols=160, cap=CAP, lm_cap=LM_CAP, kp_cap=KP_CAP, pitch=None, good=KC.GOOD, bad=KC.BAD, stream=None, stride=None):
        import torch
        self.torch, self.api, self.S, self.rows, self.cols, self.cap, self.lm_cap, self.kp_cap = torch, api, S, rows, cols, cap, lm_cap, kp_cap
        self.K = TC.K_of(rows, cols)
        self.trk = api.Tracker(S, rows, cols, cap, lm_cap, self.K, good, bad, stream=stream)
        self.pitch = pitch or cols
        self.stride = stride or rows * self.pitch + 32
        z = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device="cuda")
        dims = {"cap": cap, "cap2": 2 * cap}
        self.out = {k: z((S,) + tuple(dims.get(d, d) for d in shp), dt) for k, (shp, dt) in OUT_SPEC.items()}
        self.d_right = z((S, self.stride), "uint8"); self.d_kps = z((S, kp_cap, 28), "uint8"); self.d_n = z((S,), "int32")
        self.cases = [None] * S

    def load(self, s, case, why=KR.WHY_KEYFRAME, ids=True):
        self.trk.set_frame(s, case["st"], image=case["left"])
        if ids:
            i = case["ids"]
            self.trk.set_ids(s, i["landmark_id"], i["ref_kf_id"], i["next_kf_id"], i["next_mp_id"])
        if why:
            self.trk.debug_freeze(s, why)
        self.cases[s] = dict(case, why=why or KR.WHY_NONE)

    def state(self, s):
        """get_frame with the stored image (a stream that was never set has none: zeros stand in)"""
        if self.cases[s] is None:
            return dict(self.trk.get_frame(s), image=np.zeros((self.rows, self.cols), np.uint8))
        return self.trk.get_frame(s, image=True)

    def pre(self, s):
        return dict(self.state(s), why=self.cases[s]["why"] if self.cases[s] else KR.WHY_NONE), self.trk.get_ids(s)

    def stage(self, n_new=None):
        """right images and detected key-points of the loaded cases -> device"""
        right = np.zeros((self.S, self.stride), np.uint8); kps = np.zeros((self.S, self.kp_cap), self.api.KP_DTYPE); n = np.zeros(self.S, np.int32)
        for s, c in enumerate(self.cases):
            if c is None:
                continue
            r = right[s, :self.rows * self.pitch].reshape(self.rows, self.pitch)
            r[:, :self.cols] = c["right"]; r[:, self.cols:] = 0xEE
            k = len(c["new_xy"])
            kps["x"][s, :k], kps["y"][s, :k] = c["new_xy"][:, 0], c["new_xy"][:, 1]
            kps["size"][s], kps["octave"][s], kps["class_id"][s] = 31.0, 3, -7          # never read
            n[s] = k
        if n_new is not None:
            n[:] = n_new
        self.d_right.copy_(self.torch.from_numpy(right)); self.d_kps.copy_(self.torch.from_numpy(kps.view(np.uint8).reshape(self.S, self.kp_cap, 28)))
        self.d_n.copy_(self.torch.from_numpy(n))
        for v in self.out.values():
            v.fill_(0)
        self.torch.cuda.synchronize()

    def enqueue(self):
        self.trk.keyframe_batch(self.d_right.data_ptr(), self.pitch, self.stride, self.d_kps.data_ptr(), self.d_n.data_ptr(), self.kp_cap, B,
                                {k: v.data_ptr() for k, v in self.out.items()})

    def turn(self, n_new=None):
        self.stage(n_new)
        self.enqueue()
        self.torch.cuda.synchronize()
        return self.results()

    def results(self):
        return {k: v.cpu().numpy() for k, v in self.out.items()}


def check_stream(pkg, rig, s, pre, out, lk, new_xy=None):
    """stream s of a finished turn against the walk from `pre` = (state, ids) downloaded before it; returns the report"""
    chain, api, c = pkg.chain, rig.api, rig.cases[s]
    st, ids = pre
    new_xy = (c["new_xy"] if c is not None else np.zeros((0, 2), np.float32)) if new_xy is None else new_xy
    tag = f"stream {s} ({c['name'] if c else 'never set'})"
    post, pids = rig.state(s), rig.trk.get_ids(s)
    rep = out["report"][s]
    if not KR.eligible(st, ids) or len(st["lm"]) + len(new_xy) > rig.cap:
        w_post, w_ids, w_out = KR.turn(chain, rig.K, B, st, ids, new_xy, None, None, None, None, rig.cap, rig.lm_cap)
    else:
        p0, p1, lm = KR.append_and_starts(chain, rig.K, B, st, new_xy)
        d_p0, rxy, rok, txyz, tok = rig.trk.debug_last_turn(s)
        assert _same(d_p0, p0), tag + ": appended table"
        if len(p0):                                    # LK: the bits of myslam_lk_track on the same images, points and start points
            nxt, ok, _ = lk.track(st["image"], c["right"], p0, p1)
            assert np.array_equal(ok, rok) and _same(nxt[ok], rxy[rok]), tag + ": right tracks are not myslam_lk_track's bits"
        cand = KR.candidates(lm, rok)
        if cand:                                       # triangulation: the bits of myslam_triangulate_stereo on the same pixels
            xyz, o = api.triangulate_stereo(p0[cand, 0], p0[cand, 1], rxy[cand, 0], rxy[cand, 1], *rig.K, B)
            assert np.array_equal(o.astype(bool), tok[cand]) and _same(xyz, txyz[cand]), tag + ": triangulation is not myslam_triangulate_stereo's bits"
        assert not tok[[i for i in range(len(p0)) if i not in set(cand)]].any()
        w_post, w_ids, w_out = KR.turn(chain, rig.K, B, st, ids, new_xy, rxy, rok, txyz, tok, rig.cap, rig.lm_cap)
    assert rep.tolist() == w_out["report"].tolist(), tag + f": report {rep.tolist()} vs {w_out['report'].tolist()}"
    assert out["new_kf_id"][s] == w_out["new_kf_id"] and out["n_feat"][s] == w_out["n_feat"] and out["n_outlier_mp"][s] == w_out["n_outlier_mp"], tag
    if rep[0] == 0:
        m, no = w_out["n_feat"], w_out["n_outlier_mp"]
        for k in ("feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags"):
            assert _same(out[k][s, :m], w_out[k]), tag + ": " + k
        assert _same(out["new_kf_pose"][s], w_out["new_kf_pose"]), tag + ": key-frame pose"
        assert _same(out["outlier_mp_id"][s, :no], w_out["outlier_mp_id"]), tag + ": outlier ids"
        assert _same(out["right_ok"][s, :m].astype(bool), w_out["right_ok"]) and _same(out["right_xy"][s, :m][w_out["right_ok"]], w_out["right_xy"][w_out["right_ok"]])
        w_post = dict(w_post, image=st["image"])       # the stored left image stays
    for k in STATE_KEYS:
        assert _same(post[k], np.asarray(w_post[k], np.asarray(post[k]).dtype)), tag + ": state " + k
    for k in pids:
        assert _same(pids[k], np.asarray(w_ids[k], np.asarray(pids[k]).dtype)), tag + ": ids " + k
    return rep


def run_and_check(pkg, rig, lk):
    pre = [rig.pre(s) for s in range(rig.S)]
    out = rig.turn()
    return out, [check_stream(pkg, rig, s, pre[s], out, lk) for s in range(rig.S)]


@pytest.fixture(scope="module")
def lk(api):
    return api.LKTracker()


# ------------------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("rows,cols,pitch", [(120, 160, 167), (118, 157, 157), (117, 160, 160)])
def test_masks_are_the_walks_bytes(api, pkg, rows, cols, pitch):
    import torch
    chain, cap = pkg.chain, 300
    tabs = KC.mask_tables(rows, cols, cap)
    names = list(tabs)
    S = len(names) + 4
    trk = api.Tracker(S, rows, cols, cap, 8, TC.K_of(rows, cols), 20, 10)
    img = np.zeros((rows, cols), np.uint8)
    states = []
    for s, nm in enumerate(names):
        st = KC.table_state(chain, tabs[nm])
        trk.set_frame(s, st, image=img); trk.set_ids(s, [], 0, 1, 0); trk.debug_freeze(s, KR.WHY_KEYFRAME)
        states.append((dict(st, frozen=1, why=KR.WHY_KEYFRAME), {"valid": 1}))
    busy = KC.table_state(chain, tabs["overlap"])
    s0 = len(names)                                   # not eligible: running; frozen LOST; ids not valid; never set
    trk.set_frame(s0, busy, image=img); trk.set_ids(s0, [], 0, 1, 0)
    trk.set_frame(s0 + 1, busy, image=img); trk.set_ids(s0 + 1, [], 0, 1, 0); trk.debug_freeze(s0 + 1, KR.WHY_LOST)
    trk.set_frame(s0 + 2, busy, image=img); trk.debug_freeze(s0 + 2, KR.WHY_KEYFRAME)
    stride = rows * pitch + 64
    d = torch.full((S, stride), 0x77, dtype=torch.uint8, device="cuda")
    trk.keyframe_masks(d.data_ptr(), pitch, stride)
    got = d.cpu().numpy()
    for s in range(S):
        m = got[s, :rows * pitch].reshape(rows, pitch)
        want = KR.mask(rows, cols, *states[s]) if s < len(names) else np.zeros((rows, cols), np.uint8)
        assert _same(m[:, :cols], want), names[s] if s < len(names) else f"ineligible {s}"
        assert (m[:, cols:] == 0x77).all() and (got[s, rows * pitch:] == 0x77).all(), "bytes outside the mask were written"
    assert got[names.index("half"), :rows * pitch].reshape(rows, pitch)[50, 29:31].tolist() == [255, 0]          # rint(30.5) = 30 (half up: 31)
    assert got[names.index("empty"), :rows * pitch].reshape(rows, pitch)[:, :cols].min() == 255
    with pytest.raises(api.MyslamError):
        trk.keyframe_masks(d.data_ptr(), cols - 1, stride)
    with pytest.raises(api.MyslamError):
        trk.keyframe_masks(0, pitch, stride)


# ------------------------------------------------------------------------------------------------------------------------ the turn
def test_turn_rich_disparities_and_neighbours(api, pkg, synth, lk):
    chain = pkg.chain
    rig = Rig(api, 4, pitch=163)
    cases = [KC.rich_case(chain, synth)] + KC.disparity_cases(chain, synth)
    rig.load(2, cases[0]); rig.load(0, cases[1]); rig.load(3, cases[2])          # stream 1 never set
    out, reps = run_and_check(pkg, rig, lk)
    assert reps[2][0] == 0 and reps[2][4] >= 10 and reps[1][0] == api.Tracker.NO_TURN and reps[3][4] == 0
    assert rig.trk.keyframe_launches() == 3 + 3 and rig.trk.launches_per_step() == 5 + 3
    _cache["rich"] = ({k: v[2].copy() for k, v in out.items()}, _state_bytes(rig.trk.get_frame(2, image=True), rig.trk.get_ids(2)))
    # a second turn without a step in between: nobody is frozen any more, nothing moves
    before = [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(4)]
    out2 = rig.turn()
    assert (out2["report"][:, 0] == api.Tracker.NO_TURN).all() and (out2["new_kf_id"] == -1).all() and (out2["n_feat"] == 0).all()
    assert [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(4)] == before


def test_a_streams_bytes_do_not_depend_on_its_slot_or_neighbours(api, pkg, synth, lk):
    if "rich" not in _cache:
        test_turn_rich_disparities_and_neighbours(api, pkg, synth, lk)
    rig = Rig(api, 1)
    rig.load(0, KC.rich_case(pkg.chain, synth))
    out, reps = run_and_check(pkg, rig, lk)
    want_out, want_state = _cache["rich"]
    n = int(out["n_feat"][0])
    for k, v in out.items():
        a, b = v[0], want_out[k]
        if k.startswith("feat_") or k.startswith("right_"):
            a, b = a[:n], b[:n]
        assert _same(a, b) or (k == "right_xy" and _same(a[out["right_ok"][0, :n] != 0], b[out["right_ok"][0, :n] != 0])), k
    assert _state_bytes(rig.trk.get_frame(0, image=True), rig.trk.get_ids(0)) == want_state


def test_turn_counts_on_the_rounds_of_256_and_cap(api, pkg, synth, lk):
    chain = pkg.chain
    cases = [KC.total_case(chain, synth, t, seed=k) for k, t in enumerate(KC.TOTALS)] + [KC.total_case(chain, synth, CAP + 1, seed=20)]
    rig = Rig(api, len(cases))
    for s, c in enumerate(cases):
        rig.load(s, c)
    out, reps = run_and_check(pkg, rig, lk)
    assert [int(r[5]) for r in reps[:-1]] == KC.TOTALS and all(r[0] == 0 for r in reps[:-1])
    assert reps[-1][0] == api.ERR_CAPACITY and rig.trk.get_frame(len(cases) - 1)["frozen"] == 1          # cap exceeded by one: untouched (check_stream), still frozen
    assert reps[KC.TOTALS.index(CAP)][5] == CAP                                                          # cap met exactly
    # n_new = 0, below 0 (reads as 0) and above kp_cap (reads as kp_cap)
    for s, c in enumerate(cases):
        rig.load(s, c)
    pre = [rig.pre(s) for s in range(rig.S)]
    n_new = np.zeros(rig.S, np.int32); n_new[1::3] = -5; n_new[2] = KP_CAP + 9
    out = rig.turn(n_new)
    for s in range(rig.S):
        k = KP_CAP if n_new[s] > KP_CAP else 0
        xy = np.zeros((KP_CAP, 2), np.float32); xy[:len(cases[s]["new_xy"])] = cases[s]["new_xy"]
        rep = check_stream(pkg, rig, s, pre[s], out, lk, new_xy=xy[:k])
        assert rep[2] == k and rep[0] == 0


def test_turn_se3_branches(api, pkg, synth, lk):
    cases = KC.se3_cases(pkg.chain, synth)
    rig = Rig(api, len(cases))
    for s, c in enumerate(cases):
        rig.load(s, c)
    out, reps = run_and_check(pkg, rig, lk)
    assert all(r[0] == 0 and r[4] >= 6 for r in reps)


@pytest.mark.parametrize("k", [1, 2])
def test_turn_odd_sizes(api, pkg, synth, lk, k):
    rows, cols = TC.SIZES[k]
    rig = Rig(api, 2, rows, cols, pitch=cols + 5)
    rig.load(1, KC.size_cases(pkg.chain, synth)[k])
    out, reps = run_and_check(pkg, rig, lk)
    assert reps[1][0] == 0 and reps[1][4] >= 10 and reps[0][0] == api.Tracker.NO_TURN


WORD_PITCH, WORD_STRIDE = 164, 120 * 164 + 33     # rows of whole words; the odd stride puts stream 1's image on an odd address


def test_turn_copies_words_and_bytes_in_one_launch(api, pkg, synth, lk):
    """the image copy moves 4-byte words when the widths and the stream's own source base allow it: stream 0 does, stream 1 (odd base) moves bytes.
    The right image is only seen through LK: check_stream holds the right tracks to myslam_lk_track's bits on the unpadded images"""
    rig = Rig(api, 2, pitch=WORD_PITCH, stride=WORD_STRIDE)
    assert rig.d_right.data_ptr() % 4 == 0 and (rig.d_right.data_ptr() + rig.stride) % 4 != 0
    rig.load(0, KC.rich_case(pkg.chain, synth)); rig.load(1, KC.make(pkg.chain, synth, "odd_base", n=40, n_new=24, seed=270, no_lm=(6, 7)))
    out, reps = run_and_check(pkg, rig, lk)
    assert all(r[0] == 0 and r[3] >= 30 and r[4] >= 10 for r in reps), [r.tolist() for r in reps]
    for s in range(2):                                   # the stored left image stays, and no pad byte of the right image's rows reached it
        assert _same(rig.trk.get_frame(s, image=True)["image"], rig.cases[s]["left"])


def test_landmark_cap_met_exactly_and_exceeded_by_one(api, pkg, synth, lk):
    if "rich" not in _cache:
        test_turn_rich_disparities_and_neighbours(api, pkg, synth, lk)
    full = int(_cache["rich"][0]["report"][6])
    case = KC.rich_case(pkg.chain, synth)
    assert len(case["st"]["lm_pos"]) <= full - 1
    for lm_cap, status in ((full, 0), (full - 1, api.ERR_CAPACITY)):
        rig = Rig(api, 2, lm_cap=lm_cap)
        rig.load(0, case); rig.load(1, KC.disparity_cases(pkg.chain, synth)[1])
        out, reps = run_and_check(pkg, rig, lk)          # (a refused stream keeps every byte: check_stream compares the whole state)
        assert reps[0][0] == status and reps[1][0] == 0
        assert rig.trk.get_frame(0)["frozen"] == (1 if status else 0)


def test_ineligible_streams_are_untouched_and_a_stepped_stream_takes_its_turn(api, pkg, synth, lk):
    """the step's tail records why it froze a stream: LOST, capacity and never-set streams take no turn, a stream frozen by the key-frame rule
    without ids takes none either; the same stream with ids does, and its outlier list (filled by the step) comes out as ids"""
    import torch
    chain = pkg.chain
    rig = Rig(api, 6, cap=64, good=20, bad=10)
    kf = TC.make(chain, synth, "stepped", n=48, seed=31, outliers=(3, 17, 30), kf_every=1, ref_frame_id=9, next_frame_id=10)
    lost = TC.make(chain, synth, "lost", n=0, seed=32, kf_every=0)
    big = TC.make(chain, synth, "overflow", n=65, seed=33)
    turn_of = lambda c, nm: dict(name=nm, st=c["st"], ids=KC.ids_of(len(c["st"]["lm_pos"])), left=c["prev"], right=TC.images(synth, 31, 120, 160, (3, 0))[1],
                                 new_xy=KC.new_points(120, 160, 10, 31))
    rig.load(0, turn_of(kf, "kf_with_ids"), why=0)
    rig.load(1, turn_of(kf, "kf_without_ids"), why=0, ids=False)
    rig.load(2, turn_of(lost, "lost"), why=0)
    with pytest.raises(api.MyslamError):
        rig.load(3, turn_of(big, "overflow"), why=0, ids=False)
    rig.cases[3] = dict(turn_of(big, "overflow"), why=0)
    rig.load(4, turn_of(TC.make(chain, synth, "running", n=40, seed=34, kf_every=0), "running"), why=0)          # stream 5 never set
    d_img = torch.from_numpy(np.stack([kf["cur"], kf["cur"], lost["cur"], big["cur"], rig.cases[4]["left"], lost["cur"]])).cuda()
    d_res = torch.zeros(6 * 80, dtype=torch.uint8, device="cuda")
    rig.trk.step_batch(d_img.data_ptr(), 160, 120 * 160, d_res.data_ptr())
    res = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert res["needs_host"][:5].tolist() == [1, 1, 1, 1, 0] and res["status"][2] == chain.LOST and res["status"][3] == api.ERR_CAPACITY
    for s in range(5):
        rig.cases[s]["why"] = KR.why_of(res[s])
        rig.cases[s]["left"] = d_img[s].cpu().numpy()          # the stored image is the step's
    assert [rig.cases[s]["why"] for s in range(5)] == [KR.WHY_KEYFRAME, KR.WHY_KEYFRAME, KR.WHY_LOST, KR.WHY_CAPACITY, KR.WHY_NONE]
    pre = [rig.pre(s) for s in range(6)]
    assert len(pre[0][0]["outlier_list"]) >= 2 and pre[0][1]["valid"] == 1 and pre[1][1]["valid"] == 0
    # masks: only stream 0 is eligible
    d_m = torch.zeros((6, 120, 160), dtype=torch.uint8, device="cuda")
    rig.trk.keyframe_masks(d_m.data_ptr(), 160, 120 * 160)
    m = d_m.cpu().numpy()
    assert _same(m[0], KR.mask(120, 160, *pre[0])) and m[0].max() == 255 and not m[1:].any()
    out = rig.turn()
    reps = [check_stream(pkg, rig, s, pre[s], out, lk) for s in range(6)]
    assert reps[0][0] == 0 and out["n_outlier_mp"][0] == len(pre[0][0]["outlier_list"]) and [r[0] for r in reps[1:]] == [api.Tracker.NO_TURN] * 5
    # the running stream steps on as if no turn had been enqueued beside it; the turned stream tracks from its key-frame
    rig.trk.step_batch(d_img.data_ptr(), 160, 120 * 160, d_res.data_ptr())
    res2 = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert res2["frame_id"][4] == res["frame_id"][4] + 1 and res2["frame_id"][0] == res["frame_id"][0] + 1 and res2["n_features"][0] >= 40
    assert res2[1:4].tobytes() == res[1:4].tobytes()


def test_call_level_refusals(api, pkg, synth):
    rig = Rig(api, 1)
    rig.load(0, KC.rich_case(pkg.chain, synth))
    rig.stage()
    before = _state_bytes(rig.trk.get_frame(0, image=True), rig.trk.get_ids(0))
    ptrs = {k: v.data_ptr() for k, v in rig.out.items()}
    for kw in ({"step": rig.cols - 1}, {"kp_cap": 0}, {"d_right": 0}, {"d_new_kps": 0}, {"out": dict(ptrs, report=0)}):
        a = dict(d_right=rig.d_right.data_ptr(), step=rig.pitch, stride=rig.stride, d_new_kps=rig.d_kps.data_ptr(), d_n_new=rig.d_n.data_ptr(), kp_cap=KP_CAP,
                 baseline=B, out=ptrs)
        a.update(kw)
        with pytest.raises(api.MyslamError) as e:
            rig.trk.keyframe_batch(**a)
        assert e.value.code == api.ERR_INVALID
    assert _state_bytes(rig.trk.get_frame(0, image=True), rig.trk.get_ids(0)) == before
    ids = KC.rich_case(pkg.chain, synth)["ids"]
    for bad in (dict(landmark_id=ids["landmark_id"][:-1]), dict(landmark_id=-ids["landmark_id"]), dict(next_mp_id=int(ids["landmark_id"].max())), dict(ref_kf_id=-1)):
        a = dict(ids); a.update(bad)
        with pytest.raises(api.MyslamError):
            rig.trk.set_ids(0, a["landmark_id"], a["ref_kf_id"], a["next_kf_id"], a["next_mp_id"])
    rig.trk.set_frame(0, rig.cases[0]["st"], image=rig.cases[0]["left"])
    assert rig.trk.get_ids(0)["valid"] == 0, "set_frame clears the ids"


def test_recorded_turn_replayed_twice_equals_the_eager_turn(api, pkg, synth, lk):
    import torch
    chain = pkg.chain
    s_main, s_side = torch.cuda.Stream(), torch.cuda.Stream()
    rig = Rig(api, 3, stream=s_main.cuda_stream)
    cases = [KC.rich_case(chain, synth), KC.total_case(chain, synth, 257), KC.se3_cases(chain, synth)[3]]

    def reset():
        for s, c in enumerate(cases):
            rig.load(s, c)
        rig.stage()
    dump = lambda: [rig.results()[k].tobytes() for k in sorted(rig.out) if k not in ("right_xy", "feat_mp_pos", "feat_mp_id", "feat_uv", "feat_tag", "feat_flags")] + \
        [rig.results()[k][s, :int(rig.results()["n_feat"][s])].tobytes() for s in range(3) for k in ("feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag")] + \
        [b for s in range(3) for b in _state_bytes(rig.state(s), rig.trk.get_ids(s))]
    reset(); rig.enqueue(); torch.cuda.synchronize()
    eager = dump()
    reset()
    g = api.StepGraph.record(s_main.cuda_stream, [s_side.cuda_stream], rig.enqueue)
    assert g.node_count() >= rig.trk.keyframe_launches()
    assert (rig.results()["report"] == 0).all() and rig.trk.get_frame(0)["frozen"] == 1, "recording a turn must not run it"
    for _ in range(2):
        g.launch(s_main.cuda_stream); torch.cuda.synchronize()
        assert dump() == eager
        reset()


# ------------------------------------------------------------------------------------------------------------------------ update, set image
def test_update_from_map_and_set_image(api, pkg, synth, lk):
    import torch
    chain = pkg.chain
    rig = Rig(api, 4, good=20, bad=10)
    cases = [KC.make(chain, synth, f"upd{s}", n=30, n_new=0, seed=240 + s, shared=((1, 2),)) for s in range(4)]
    rig.load(0, cases[0], why=0); rig.load(1, cases[1], why=0); rig.load(2, cases[2], why=KR.WHY_KEYFRAME); rig.load(3, cases[3], why=0, ids=False)
    kf_cap, mp_cap = 6, 64
    rng = np.random.default_rng(9)
    kf_id = np.full((4, kf_cap), -1, np.int64); kf_pose = np.zeros((4, kf_cap, 7)); n_kf = np.zeros(4, np.int32)
    mp_id = np.full((4, mp_cap), -1, np.int64); mp_pos = np.zeros((4, mp_cap, 3)); mp_out = np.zeros((4, mp_cap), np.uint8); n_mp = np.zeros(4, np.int32)
    lid = cases[0]["ids"]["landmark_id"]
    for s in range(4):
        # stream 0: the ref key-frame is the LAST row, landmark ids on the first and the last row, some absent; stream 1: the ref key-frame is gone
        rows = [3, 5, 7] if s != 1 else [3, 5, 8]
        kf_id[s, :3] = rows; kf_pose[s, :3] = [TC.pose7(TC.quat((0.1, 1, 0.2), 3.0 + r), (0.1 * r, 0.2, -0.3)) for r in rows]; n_kf[s] = 3
        have = np.sort(np.concatenate([lid[[0, 4, 9, 29]], [lid[9] + 1]]))          # the tracker's ids 0 (first row), 4, 9, 29 (last row); one id it does not hold
        mp_id[s, :len(have)] = have; mp_pos[s, :len(have)] = rng.uniform(-5, 5, (len(have), 3)); mp_out[s, :len(have)] = rng.integers(0, 2, len(have)); n_mp[s] = len(have)
    mp_id[0, n_mp[0]] = lid[10]                                                                     # a row beyond the count is not part of the table
    dev = [torch.from_numpy(a).cuda() for a in (kf_id, kf_pose, n_kf, mp_id, mp_pos, mp_out, n_mp)]
    pre = [rig.pre(s) for s in range(4)]
    rig.trk.update_from_map(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), kf_cap, dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(),
                            dev[6].data_ptr(), mp_cap)
    moved = 0
    for s in range(4):
        st, ids = pre[s]
        want = KR.update_from_map(st, ids, kf_id[s, :n_kf[s]], kf_pose[s, :n_kf[s]], mp_id[s, :n_mp[s]], mp_pos[s, :n_mp[s]], mp_out[s, :n_mp[s]])
        post = rig.state(s)
        for k in STATE_KEYS:
            assert _same(post[k], np.asarray(want[k], np.asarray(post[k]).dtype)), (s, k)
        moved += int(not _same(post["lm_pos"], st["lm_pos"]))
    p0, p1 = rig.trk.get_frame(0), rig.trk.get_frame(1)
    assert moved == 2 and _same(p0["ref_pose"], kf_pose[0, 2]) and _same(p1["ref_pose"], pre[1][0]["ref_pose"])          # frozen and id-less streams skipped
    assert _same(p0["lm_pos"][29], mp_pos[0, list(mp_id[0, :n_mp[0]]).index(lid[29])]) and _same(p0["lm_pos"][10], pre[0][0]["lm_pos"][10])
    # set_image_batch: equals set_frame(prev_image=...) byte for byte, pyramid included (one following step shows it)
    a, b = Rig(api, 3, good=20, bad=10), Rig(api, 3, good=20, bad=10)
    new_img = [TC.images(synth, 250 + s, 120, 160, (1, 0))[1] for s in range(3)]
    nxt_img = torch.from_numpy(np.stack([TC.images(synth, 250 + s, 120, 160, (2, 0))[1] for s in range(3)])).cuda()
    for s in range(3):
        c = KC.make(chain, synth, f"img{s}", n=30, n_new=0, seed=250 + s)
        a.load(s, c, why=0); b.load(s, c, why=0)
        if s != 1:
            b.trk.set_frame(s, c["st"], image=new_img[s]); b.trk.set_ids(s, **{k: c["ids"][k] for k in c["ids"]})
    pitch = 171
    pad = np.full((3, 120, pitch), 0xAB, np.uint8)
    for s in range(3):
        pad[s, :, :160] = new_img[s]
    d_pad = torch.from_numpy(pad).cuda(); sel = torch.from_numpy(np.array([1, 0, 7], np.uint8)).cuda()
    a.trk.set_image_batch(d_pad.data_ptr(), pitch, 120 * pitch, sel.data_ptr())
    ra, rb = torch.zeros(3 * 80, dtype=torch.uint8, device="cuda"), torch.zeros(3 * 80, dtype=torch.uint8, device="cuda")
    for s in range(3):
        assert _state_bytes(a.trk.get_frame(s, image=True), a.trk.get_ids(s)) == _state_bytes(b.trk.get_frame(s, image=True), b.trk.get_ids(s))
    a.trk.step_batch(nxt_img.data_ptr(), 160, 120 * 160, ra.data_ptr()); b.trk.step_batch(nxt_img.data_ptr(), 160, 120 * 160, rb.data_ptr())
    assert ra.cpu().numpy().tobytes() == rb.cpu().numpy().tobytes()
    for s in range(3):
        assert _state_bytes(a.trk.get_frame(s, image=True), a.trk.get_ids(s)) == _state_bytes(b.trk.get_frame(s, image=True), b.trk.get_ids(s))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.trk.debug_last_step(s), b.trk.debug_last_step(s)))


def test_set_image_copies_words_and_bytes_in_one_launch(api, pkg, synth):
    """set_image_batch with rows of whole words: stream 0's source base is 4-byte aligned (word copy), stream 1's is odd (byte copy).  Both equal
    set_frame(prev_image=...) byte for byte, pyramid included (one following step shows it), so no 0xAB pad byte reached a stored image"""
    import torch
    chain = pkg.chain
    a, b = Rig(api, 2, good=20, bad=10), Rig(api, 2, good=20, bad=10)
    new_img = [TC.images(synth, 260 + s, 120, 160, (1, 0))[1] for s in range(2)]
    nxt_img = torch.from_numpy(np.stack([TC.images(synth, 260 + s, 120, 160, (2, 0))[1] for s in range(2)])).cuda()
    for s in range(2):
        c = KC.make(chain, synth, f"wimg{s}", n=30, n_new=0, seed=260 + s)
        a.load(s, c, why=0); b.load(s, c, why=0)
        b.trk.set_frame(s, c["st"], image=new_img[s]); b.trk.set_ids(s, **{k: c["ids"][k] for k in c["ids"]})
    pad = np.full((2, WORD_STRIDE), 0xAB, np.uint8)
    for s in range(2):
        pad[s, :120 * WORD_PITCH].reshape(120, WORD_PITCH)[:, :160] = new_img[s]
    d_pad = torch.from_numpy(pad).cuda(); sel = torch.from_numpy(np.array([1, 1], np.uint8)).cuda()
    assert d_pad.data_ptr() % 4 == 0 and (d_pad.data_ptr() + WORD_STRIDE) % 4 != 0
    a.trk.set_image_batch(d_pad.data_ptr(), WORD_PITCH, WORD_STRIDE, sel.data_ptr())
    ra, rb = torch.zeros(2 * 80, dtype=torch.uint8, device="cuda"), torch.zeros(2 * 80, dtype=torch.uint8, device="cuda")
    for s in range(2):
        assert _same(a.trk.get_frame(s, image=True)["image"], new_img[s]), f"stream {s}: stored image"
        assert _state_bytes(a.trk.get_frame(s, image=True), a.trk.get_ids(s)) == _state_bytes(b.trk.get_frame(s, image=True), b.trk.get_ids(s))
    a.trk.step_batch(nxt_img.data_ptr(), 160, 120 * 160, ra.data_ptr()); b.trk.step_batch(nxt_img.data_ptr(), 160, 120 * 160, rb.data_ptr())
    assert ra.cpu().numpy().tobytes() == rb.cpu().numpy().tobytes()
    for s in range(2):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.trk.debug_last_step(s), b.trk.debug_last_step(s)))
