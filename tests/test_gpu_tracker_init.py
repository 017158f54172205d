"""StereoInit of the multi-stream tracker on the GPU (csrc/tracker.hip: myslam_tracker_reset_stream / _init_masks / _init_batch) against
tests/tracker_init_ref.py, the walk that tests/test_tracker_init_ref.py pins to the chain.  The walk is fed the device's right tracks and the
device's triangulation — themselves checked bit for bit against myslam_lk_track and myslam_triangulate_stereo on the same images and points —
and the report, the outputs and the whole post-state (get_frame, get_ids) must be its bytes (tracker_init_ref.check_item).  get_frame hands out
a stored image only for a stream that was given one through set_frame, so the stored image is compared on streams that were set and then reset
(`mark`); for a stream straight from create, the step that follows the init shows it.  Hand-made pairs at 120 x 160 and 118 x 157."""
import numpy as np
import pytest

import tracker_cases as TC
import tracker_init_ref as IR
import tracker_kf_cases as KC
import tracker_kf_ref as KR
from test_gpu_tracker_kf import Rig, _same, _state_bytes, check_stream

pytestmark = pytest.mark.gpu

B = KC.BASELINE


def pair(synth, name, m, seed, d=3, rows=120, cols=160, lose=False):
    """a stereo pair (the right image is the left one moved by d pixels: disparity d) and m detected key-points.  lose: every fifth key-point
    from the fourth on sits at the left border, where its right match lies outside the image, and every eleventh from the fifth on has a NaN
    row: lost tracks and failed triangulations between the successes, so that ranks and indices part"""
    left, right = TC.images(synth, seed, rows, cols, (d, 0))
    xy = KC.new_points(rows, cols, m, seed)
    if lose:
        xy[3::5, 0] = np.float32(1.25); xy[4::11, 1] = np.float32(np.nan)
    return {"name": name, "left": left, "right": right, "new_xy": xy, "why": KR.WHY_NONE, "d": d}


class InitRig(Rig):
    """Rig with the left images on the device as well; cases of streams that take an init are pair()s.  left_offset: the left images start
    that many bytes into their allocation, so that a left image's address can be aligned where its right image's is not, and the reverse"""

    def __init__(self, api, chain, S, left_offset=0, **kw):
        super().__init__(api, S, **kw)
        self.chain, self.marked = chain, set()
        self.left_store = self.torch.zeros(left_offset + S * self.stride, dtype=self.torch.uint8, device="cuda")
        self.d_left = self.left_store[left_offset:].view(S, self.stride)

    def arm(self, s, case, mark=None):
        """stream s will see `case`; mark = reset_stream's counters: the stream is given a (black) image through set_frame first, so that
        get_frame can download the stored image afterwards, and is then put back into the created state"""
        if mark is not None:
            self.trk.set_frame(s, KC.table_state(self.chain, np.zeros((0, 2), np.float32)), image=np.zeros((self.rows, self.cols), np.uint8))
            self.trk.reset_stream(s, *mark)
            self.marked.add(s)
        self.cases[s] = dict(case)

    def load(self, s, case, **kw):
        super().load(s, case, **kw)
        self.marked.add(s)

    def state(self, s):
        if s in self.marked:
            return self.trk.get_frame(s, image=True)
        return dict(self.trk.get_frame(s), image=np.zeros((self.rows, self.cols), np.uint8))

    def stage(self, n_new=None):
        left = np.zeros((self.S, self.stride), np.uint8)
        for s, c in enumerate(self.cases):
            if c is not None:
                l = left[s, :self.rows * self.pitch].reshape(self.rows, self.pitch)
                l[:, :self.cols] = c["left"]; l[:, self.cols:] = 0xDD
        self.d_left.copy_(self.torch.from_numpy(left))
        super().stage(n_new)

    def enqueue_init(self, init_good):
        self.trk.init_batch(self.d_left.data_ptr(), self.d_right.data_ptr(), self.pitch, self.stride, self.d_kps.data_ptr(), self.d_n.data_ptr(), self.kp_cap, B,
                            init_good, {k: v.data_ptr() for k, v in self.out.items()})

    def init(self, init_good, n_new=None):
        self.stage(n_new)
        self.enqueue_init(init_good)
        self.torch.cuda.synchronize()
        return self.results()


def check_init(rig, s, pre, out, lk, init_good, new_xy=None):
    """stream s of a finished init_batch against the walk from `pre` = (state, ids) downloaded before it; returns the report"""
    api, c = rig.api, rig.cases[s]
    st, ids = pre
    new_xy = (c["new_xy"] if c is not None else np.zeros((0, 2), np.float32)) if new_xy is None else new_xy
    tag = f"stream {s} ({c['name'] if c else 'never set'})"
    post, pids = rig.state(s), rig.trk.get_ids(s)
    o = {k: v[s] for k, v in out.items()}
    image = st["image"]
    if not IR.eligible(st) or len(new_xy) > rig.cap:
        w = IR.init(st, ids, new_xy, None, None, None, None, rig.cap, rig.lm_cap, init_good)
    else:
        d_p0, rxy, rok, txyz, tok = rig.trk.debug_last_turn(s)
        assert _same(d_p0, new_xy), tag + ": feature table"
        if len(new_xy):                                # LK: the bits of myslam_lk_track on the same two images, every start point the feature's own pixel
            nxt, ok, _ = lk.track(c["left"], c["right"], new_xy, new_xy)
            assert np.array_equal(ok, rok) and _same(nxt[ok], rxy[rok]), tag + ": right tracks are not myslam_lk_track's bits"
        cand = [i for i in range(len(new_xy)) if rok[i]]
        if cand:                                       # triangulation: the bits of myslam_triangulate_stereo on the same pixels
            xyz, t_ok = api.triangulate_stereo(new_xy[cand, 0], new_xy[cand, 1], rxy[cand, 0], rxy[cand, 1], *rig.K, B)
            assert np.array_equal(t_ok.astype(bool), tok[cand]) and _same(xyz, txyz[cand]), tag + ": triangulation is not myslam_triangulate_stereo's bits"
        assert not tok[[i for i in range(len(new_xy)) if i not in set(cand)]].any()
        w = IR.init(st, ids, new_xy, rxy, rok, txyz, tok, rig.cap, rig.lm_cap, init_good)
        if s in rig.marked:
            image = c["left"]                          # the head stored the left image, whatever the tail decided
    IR.check_item(tag, post, pids, o, *w)
    assert _same(post["image"], image), tag + ": stored image"
    return o["report"]


def init_and_check(rig, lk, init_good, n_new=None):
    pre = [rig.pre(s) for s in range(rig.S)]
    out = rig.init(init_good, n_new)
    return out, [check_init(rig, s, pre[s], out, lk, init_good) for s in range(rig.S)]


@pytest.fixture(scope="module")
def lk(api):
    return api.LKTracker()


# ------------------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("rows,cols,pitch", [(120, 160, 167), (118, 157, 157)])
def test_masks_are_the_walks_bytes(api, pkg, rows, cols, pitch):
    import torch
    chain = pkg.chain
    S = 7
    trk = api.Tracker(S, rows, cols, 64, 8, TC.K_of(rows, cols), 20, 10)
    img = np.zeros((rows, cols), np.uint8)
    tab = KC.table_state(chain, KC.mask_tables(rows, cols, 64)["overlap"])
    states = [IR.created()[0]]                                                                          # 0: straight from create
    trk.set_frame(1, tab, image=img); trk.reset_stream(1, 3, 1, 9, 2); states.append(IR.reset(tab, 3, 1, 9, 2)[0])           # 1: reset
    trk.set_frame(2, tab, image=img); trk.set_ids(2, [], 0, 1, 0); trk.debug_freeze(2, KR.WHY_KEYFRAME)                     # 2: due for a turn
    states.append(dict(tab, frozen=1, why=KR.WHY_KEYFRAME))
    trk.set_frame(3, tab, image=img); states.append(dict(tab, frozen=0, why=KR.WHY_NONE))                                   # 3: running
    trk.set_frame(4, dict(tab, status=3), image=img); trk.debug_freeze(4, KR.WHY_LOST)                                      # 4: LOST
    states.append(dict(tab, status=3, frozen=1, why=KR.WHY_LOST))
    trk.set_frame(5, dict(tab, status=0), image=img); trk.debug_freeze(5, KR.WHY_KEYFRAME)                                  # 5: INITING, but a step froze it
    states.append(dict(tab, status=0, frozen=1, why=KR.WHY_KEYFRAME))
    trk.set_frame(6, dict(tab, status=0), image=img); states.append(dict(tab, status=0, frozen=0, why=KR.WHY_NONE))         # 6: INITING and running
    stride = rows * pitch + 64
    d = torch.full((S, stride), 0x77, dtype=torch.uint8, device="cuda")
    trk.init_masks(d.data_ptr(), pitch, stride)
    got = d.cpu().numpy()
    for s in range(S):
        m = got[s, :rows * pitch].reshape(rows, pitch)
        assert _same(m[:, :cols], IR.mask(rows, cols, states[s])), f"stream {s}"
        assert (m[:, cols:] == 0x77).all() and (got[s, rows * pitch:] == 0x77).all(), "bytes outside the mask were written"
    assert [int(got[s, 0]) for s in range(S)] == [255, 255, 0, 0, 0, 0, 0]
    k = torch.full((S, stride), 0x77, dtype=torch.uint8, device="cuda")            # the turn's masks see the reverse: only stream 2 is due
    trk.keyframe_masks(k.data_ptr(), pitch, stride)
    assert [int(v) for v in k.cpu().numpy()[:, :rows * pitch].reshape(S, rows, pitch)[:, :, :cols].max(axis=(1, 2))] == [0, 0, 255, 0, 0, 0, 0]
    for bad in ((d.data_ptr(), cols - 1, stride), (0, pitch, stride), (d.data_ptr(), pitch, (rows - 1) * pitch + cols - 1)):
        with pytest.raises(api.MyslamError) as e:
            trk.init_masks(*bad)
        assert e.value.code == api.ERR_INVALID


# ------------------------------------------------------------------------------------------------------------------------ the init
COUNTS = [0, 1, 255, 256, 257, 1024]


def test_init_counts_on_the_rounds_of_256_cap_and_cap_plus_one(api, pkg, synth, lk):
    chain = pkg.chain
    ms = COUNTS + [1025]
    rig = InitRig(api, chain, len(ms), kp_cap=1025, pitch=163)
    for s, m in enumerate(ms):                                           # odd streams: reset with counters of their own; even ones: straight from create
        rig.arm(s, pair(synth, f"m{m}", m, 300 + s, lose=m >= 255), mark=(10 + s, s, 1000 * s, s % 3) if s % 2 else None)
    out, reps = init_and_check(rig, lk, 0)
    assert [int(r[0]) for r in reps] == [0] * len(COUNTS) + [api.ERR_CAPACITY] and [int(r[2]) for r in reps] == ms
    assert all(r[3] >= r[4] for r in reps[:-1]) and all(r[2] > r[3] >= r[4] >= r[2] // 2 for r in reps[2:-1]), [r.tolist() for r in reps]
    assert out["new_kf_id"].tolist() == [0, 1, 0, 3, 0, 5, -1] and [int(r[1]) for r in reps] == [0, 11, 0, 13, 0, 15, 0]
    assert rig.trk.init_launches() == 3 + 2 * 3 and rig.trk.keyframe_launches() == 3 + 3
    st = rig.trk.get_frame(3)
    assert (st["status"], st["frozen"], st["kf_every"], st["next_frame_id"], st["ref_frame_id"]) == (1, 0, 0, 14, 13)
    assert rig.trk.get_ids(3)["landmark_id"][:2].tolist() == [3000, 3001]
    # again: nobody is init-eligible any more but the stream that did not fit, and that one still does not fit
    before = [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(rig.S)]
    out2, reps2 = init_and_check(rig, lk, 0)
    assert [int(r[0]) for r in reps2] == [api.Tracker.NO_TURN] * len(COUNTS) + [api.ERR_CAPACITY]
    assert [_state_bytes(rig.state(s), rig.trk.get_ids(s)) for s in range(rig.S)] == before
    # counts below 0 read as 0, above kp_cap as kp_cap (= cap + 1 here: capacity)
    rig2 = InitRig(api, chain, 3, kp_cap=1025)
    for s in range(3):
        rig2.arm(s, pair(synth, f"n{s}", 300, 320 + s), mark=(0, 0, 0, 0))
    pre = [rig2.pre(s) for s in range(3)]
    n_new = np.array([-4, 2000, 0], np.int32)
    out = rig2.init(0, n_new)
    xy = np.zeros((1025, 2), np.float32); xy[:300] = rig2.cases[1]["new_xy"]
    reps = [check_init(rig2, s, pre[s], out, lk, 0, new_xy=x) for s, x in enumerate((xy[:0], xy, xy[:0]))]
    assert [int(r[0]) for r in reps] == [0, api.ERR_CAPACITY, 0] and [int(r[2]) for r in reps] == [0, 1025, 0]


def test_init_good_met_exactly_retry_then_success_and_zero_successes(api, pkg, synth, lk):
    chain = pkg.chain
    rig = InitRig(api, chain, 4, rows=118, cols=157, pitch=160)
    cases = [pair(synth, "few", 40, 330, rows=118, cols=157), pair(synth, "many", 90, 331, rows=118, cols=157),
             pair(synth, "behind", 60, 332, d=-2, rows=118, cols=157), pair(synth, "infinity", 60, 333, d=0, rows=118, cols=157)]
    n_right = [int(np.count_nonzero(lk.track(c["left"], c["right"], c["new_xy"], c["new_xy"])[1])) for c in cases]
    assert n_right[0] <= 40 < min(n_right[2:]) <= max(n_right[2:]) <= 60 < n_right[1], n_right
    for s, c in enumerate(cases):
        rig.arm(s, c, mark=(0, 0, 0, 0))
    out, reps = init_and_check(rig, lk, n_right[1])                       # stream 1 meets init_good exactly: taken; the others retry
    want = [api.Tracker.INIT_RETRY if n < n_right[1] else 0 for n in n_right]
    assert [int(r[0]) for r in reps] == want and want[1] == 0 and want[0] == api.Tracker.INIT_RETRY
    assert [int(r[3]) for r in reps] == n_right and out["new_kf_id"][1] == 0 and out["new_kf_id"][0] == -1
    out, reps = init_and_check(rig, lk, n_right[0] + 1)                   # one above stream 0's count: it retries again
    assert reps[0].tolist()[:5] == [api.Tracker.INIT_RETRY, 1, 40, n_right[0], 0] and reps[1][0] == api.Tracker.NO_TURN
    for s in (2, 3):                                                      # a retry, then success on the next call: frame id 1, key-frame id 0
        assert reps[s].tolist()[:4] == [0, 1, 60, n_right[s]] and out["new_kf_id"][s] == 0 and rig.trk.get_frame(s)["ref_frame_id"] == 1
    out, reps = init_and_check(rig, lk, n_right[0])                       # the bound itself: taken, on its third frame, as key-frame 0
    assert reps[0].tolist()[:4] == [0, 2, 40, n_right[0]] and out["new_kf_id"][0] == 0 and rig.trk.get_frame(0)["ref_frame_id"] == 2
    # behind the cameras / at infinity: no point, and still a key-frame (BuildInitMap returns true)
    for s in (2, 3):
        st, ids = rig.trk.get_frame(s), rig.trk.get_ids(s)
        assert reps[s][0] == api.Tracker.NO_TURN and st["status"] == 1 and st["frozen"] == 0 and ids["valid"] == 1 and ids["next_kf_id"] == 1
    assert len(rig.trk.get_frame(2)["lm_pos"]) == 0 and (rig.trk.get_frame(2)["lm"] == -1).all() and len(rig.trk.get_frame(2)["lm"]) == 60
    assert rig.trk.get_ids(2)["next_mp_id"] == 0
    with np.errstate(all="ignore"):
        far = rig.trk.get_frame(3)["lm_pos"]
    assert not np.any(np.abs(far[:, 2]) < 1e3), "disparity 0: whatever the solve gives, it is not a point nearby"


def test_landmark_cap_met_exactly_and_exceeded_by_one(api, pkg, synth, lk):
    chain = pkg.chain
    case = pair(synth, "lmcap", 100, 340)
    rig = InitRig(api, chain, 1)
    rig.arm(0, case, mark=(6, 2, 50, 0))
    out, reps = init_and_check(rig, lk, 10)
    full = int(reps[0][4])
    assert reps[0][0] == 0 and 80 <= full <= 100
    for lm_cap, status in ((full, 0), (full - 1, api.ERR_CAPACITY)):
        rig = InitRig(api, chain, 2, lm_cap=lm_cap)
        rig.arm(0, case, mark=(6, 2, 50, 0)); rig.arm(1, pair(synth, "beside", 30, 341))
        before = _state_bytes(dict(rig.trk.get_frame(0), image=0), rig.trk.get_ids(0))
        out, reps = init_and_check(rig, lk, 10)           # (check_init compares the whole state with the walk's: a refused stream keeps every byte)
        assert reps[0][0] == status and reps[1][0] == 0 and reps[0][3] >= full
        if status:
            assert _state_bytes(dict(rig.trk.get_frame(0), image=0), rig.trk.get_ids(0)) == before and rig.trk.get_frame(0)["next_frame_id"] == 6
            assert out["new_kf_id"][0] == -1 and out["n_feat"][0] == 0


def test_a_streams_bytes_do_not_depend_on_its_slot_or_neighbours(api, pkg, synth, lk):
    chain = pkg.chain
    case = pair(synth, "same", 300, 350, lose=True)
    a = InitRig(api, chain, 4, pitch=171, kp_cap=700)
    a.arm(0, pair(synth, "n0", 700, 351, lose=True)); a.arm(2, case, mark=(4, 1, 77, 2)); a.arm(3, pair(synth, "n3", 5, 352, d=-1), mark=(0, 0, 0, 0))
    b = InitRig(api, chain, 1)
    b.arm(0, case, mark=(4, 1, 77, 2))
    oa, ra = init_and_check(a, lk, 20)
    ob, rb = init_and_check(b, lk, 20)
    assert [int(r[0]) for r in ra] == [0, api.Tracker.INIT_RETRY, 0, api.Tracker.INIT_RETRY] and rb[0][0] == 0          # (stream 1: never armed, no key-point)
    n = int(ob["n_feat"][0])
    assert n == 300 and ra[2].tolist() == rb[0].tolist()
    for k in oa:
        x, y = oa[k][2], ob[k][0]
        if k.startswith("feat_") or k.startswith("right_"):
            x, y = x[:n], y[:n]
        ok = ob["right_ok"][0, :n] != 0
        assert _same(x, y) or (k == "right_xy" and _same(x[ok], y[ok])), k
    assert _state_bytes(a.trk.get_frame(2, image=True), a.trk.get_ids(2)) == _state_bytes(b.trk.get_frame(0, image=True), b.trk.get_ids(0))
    assert all(_same(x, y) for x, y in zip(a.trk.debug_last_turn(2), b.trk.debug_last_turn(0)))


def test_init_copies_words_and_bytes_per_source_in_one_launch(api, pkg, synth, lk):
    """the head's image copy moves 4-byte words when the widths and that SOURCE's own base allow it.  Rows of whole words, an odd stride and the
    left images 3 bytes into their allocation: stream 0 copies its right image by words and its left image by bytes, stream 1 the reverse.
    check_init holds the right tracks to myslam_lk_track's bits on the unpadded pair and the stored image to the left input (no 0xDD, no 0xEE)"""
    from test_gpu_tracker_kf import WORD_PITCH, WORD_STRIDE
    rig = InitRig(api, pkg.chain, 2, left_offset=(-WORD_STRIDE) % 4, pitch=WORD_PITCH, stride=WORD_STRIDE)
    aligned = lambda d: [(d.data_ptr() + s * rig.stride) % 4 == 0 for s in range(2)]
    assert aligned(rig.d_right) == [True, False] and aligned(rig.d_left) == [False, True]
    for s in range(2):
        rig.arm(s, pair(synth, f"word{s}", 120, 395 + s, lose=True), mark=(s, 0, 0, 0))
    out, reps = init_and_check(rig, lk, 50)
    assert all(r[0] == 0 and r[2] == 120 and r[3] >= 60 and r[4] >= 30 for r in reps), [r.tolist() for r in reps]
    for s in range(2):
        assert _same(rig.trk.get_frame(s, image=True)["image"], rig.cases[s]["left"])


def test_init_and_turn_touch_disjoint_streams_and_the_first_step_follows(api, pkg, synth, lk):
    """a bank that mixes a stream straight from create, one due for a key-frame turn, a running one and a LOST one"""
    import torch
    chain = pkg.chain
    rig = InitRig(api, chain, 5, good=20, bad=10)
    start = pair(synth, "start", 120, 360)
    rig.arm(0, start)                                                                    # straight from create: no image to download
    rig.load(1, KC.rich_case(chain, synth))                                              # due for a turn
    rig.load(2, KC.make(chain, synth, "running", n=30, n_new=4, seed=361), why=0)
    lost = KC.make(chain, synth, "lost", n=20, n_new=4, seed=362)
    lost["st"]["status"] = 3
    rig.load(3, lost, why=KR.WHY_LOST)
    rig.arm(4, start, mark=(0, 0, 0, 0))                                                 # the same start with an image mark: its stored image is compared
    # the turn first: only stream 1 moves, the init-eligible streams keep every byte
    pre = [rig.pre(s) for s in range(5)]
    out = rig.turn()
    reps = [check_stream(pkg, rig, s, pre[s], out, lk) for s in (1, 2, 3)]
    assert [int(r[0]) for r in reps] == [0, api.Tracker.NO_TURN, api.Tracker.NO_TURN]
    for s in (0, 4):
        assert out["report"][s].tolist() == [api.Tracker.NO_TURN, -1, 120, 0, 0, 0, 0, 0] and out["new_kf_id"][s] == -1
        assert _state_bytes(rig.state(s), rig.trk.get_ids(s)) == _state_bytes(*pre[s][:1], pre[s][1]), f"the turn touched init-eligible stream {s}"
    # then the init: streams 0 and 4 start, the others keep every byte (the stream that took its turn is running now)
    out, reps = init_and_check(rig, lk, 50)
    assert [int(r[0]) for r in reps] == [0, api.Tracker.NO_TURN, api.Tracker.NO_TURN, api.Tracker.NO_TURN, 0]
    assert all(_same(out[k][0], out[k][4]) for k in out if k != "right_xy")
    assert _state_bytes(dict(rig.trk.get_frame(0), image=0), rig.trk.get_ids(0)) == _state_bytes(dict(rig.trk.get_frame(4), image=0), rig.trk.get_ids(4))
    with pytest.raises(api.MyslamError):                                                 # the host-side image mark is not the init's to set
        rig.trk.get_frame(0, image=True)
    with pytest.raises(api.MyslamError):
        rig.trk.set_frame(0, rig.trk.get_frame(0))
    # the first step of the started streams, from the stored left image and its pyramid: the next image is the pair's left one moved on by a pixel
    nxt = TC.images(synth, 360, 120, 160, (1, 0))[1]
    d_img = torch.from_numpy(np.stack([nxt, rig.cases[1]["left"], rig.cases[2]["left"], rig.cases[3]["left"], nxt])).cuda()
    d_res = torch.zeros(5 * 80, dtype=torch.uint8, device="cuda")
    rig.trk.step_batch(d_img.data_ptr(), 160, 120 * 160, d_res.data_ptr())
    res = d_res.cpu().numpy().view(api.TRACKER_RESULT_DTYPE)
    assert res[0].tobytes() == res[4].tobytes(), "the stream from create tracks from other pixels than the marked one, whose stored image was compared"
    assert res["status"][0] == chain.TRACKING_GOOD and res["frame_id"][0] == 1 and res["n_features"][0] >= reps[0][4] // 2 and res["n_inliers"][0] > 20
    assert all(_same(x, y) for x, y in zip(rig.trk.debug_last_step(0), rig.trk.debug_last_step(4)))


def test_reset_stream_after_lost(api, pkg, synth, lk):
    chain = pkg.chain
    rig = InitRig(api, chain, 2)
    lost = KC.make(chain, synth, "lost", n=25, n_new=4, seed=370)
    lost["st"]["status"] = 3
    rig.load(0, lost, why=KR.WHY_LOST); rig.load(1, KC.make(chain, synth, "beside", n=25, n_new=4, seed=371), why=0)
    pre, beside = rig.pre(0), _state_bytes(rig.state(1), rig.trk.get_ids(1))
    assert not IR.eligible(pre[0]) and pre[0]["status"] == 3 and pre[0]["frozen"] == 1
    for bad in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        with pytest.raises(api.MyslamError) as e:
            rig.trk.reset_stream(0, *bad)
        assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.MyslamError):
        rig.trk.reset_stream(2, 0, 0, 0, 0)
    assert _state_bytes(rig.state(0), rig.trk.get_ids(0)) == _state_bytes(dict(pre[0]), pre[1]), "a refused reset changed the stream"
    rig.trk.reset_stream(0, 17, 4, 333, 5)
    w_st, w_ids = IR.reset(pre[0], 17, 4, 333, 5)
    post, pids = rig.state(0), rig.trk.get_ids(0)
    for k in IR.STATE_KEYS + ("image",):
        assert _same(post[k], np.asarray(w_st[k], np.asarray(post[k]).dtype)), "reset state " + k
    assert all(_same(pids[k], np.asarray(w_ids[k], np.asarray(pids[k]).dtype)) for k in pids) and _same(post["image"], lost["left"])
    assert _state_bytes(rig.state(1), rig.trk.get_ids(1)) == beside
    rig.cases[0] = pair(synth, "restart", 80, 372)
    out, reps = init_and_check(rig, lk, 30)
    assert reps[0].tolist()[:3] == [0, 17, 80] and out["new_kf_id"][0] == 4 and reps[1][0] == api.Tracker.NO_TURN
    st, ids = rig.trk.get_frame(0), rig.trk.get_ids(0)
    assert (st["kf_every"], st["next_frame_id"], st["ref_frame_id"], st["status"]) == (5, 18, 17, 1) and ids["landmark_id"][0] == 333
    assert (ids["ref_kf_id"], ids["next_kf_id"], ids["next_mp_id"]) == (4, 5, 333 + int(reps[0][4]))


def test_call_level_refusals(api, pkg, synth):
    rig = InitRig(api, pkg.chain, 1)
    rig.arm(0, pair(synth, "refused", 50, 380), mark=(2, 1, 5, 0))
    rig.stage()
    before = _state_bytes(rig.state(0), rig.trk.get_ids(0))
    ptrs = {k: v.data_ptr() for k, v in rig.out.items()}
    for kw in ({"step": rig.cols - 1}, {"stride": (rig.rows - 1) * rig.pitch + rig.cols - 1}, {"kp_cap": 0}, {"d_left": 0}, {"d_right": 0}, {"d_new_kps": 0},
               {"d_n_new": 0}, {"out": dict(ptrs, report=0)}, {"out": dict(ptrs, new_kf_id=0)}):
        a = dict(d_left=rig.d_left.data_ptr(), d_right=rig.d_right.data_ptr(), step=rig.pitch, stride=rig.stride, d_new_kps=rig.d_kps.data_ptr(),
                 d_n_new=rig.d_n.data_ptr(), kp_cap=rig.kp_cap, baseline=B, init_good=10, out=ptrs)
        a.update(kw)
        with pytest.raises(api.MyslamError) as e:
            rig.trk.init_batch(**a)
        assert e.value.code == api.ERR_INVALID, kw
    rig.torch.cuda.synchronize()
    assert _state_bytes(rig.state(0), rig.trk.get_ids(0)) == before and not rig.results()["report"].any(), "a refused call enqueued something"
    # init_good may be any int: below 0 nothing retries, INT_MAX retries everything
    rig.enqueue_init(2**31 - 1); rig.torch.cuda.synchronize()
    assert rig.results()["report"][0, :3].tolist() == [api.Tracker.INIT_RETRY, 2, 50]
    rig.enqueue_init(-2**31); rig.torch.cuda.synchronize()
    assert rig.results()["report"][0, :3].tolist() == [0, 3, 50] and rig.results()["new_kf_id"][0] == 1


def test_recorded_init_replayed_twice_equals_the_eager_init(api, pkg, synth, lk):
    import torch
    chain = pkg.chain
    s_main, s_side = torch.cuda.Stream(), torch.cuda.Stream()
    rig = InitRig(api, chain, 3, stream=s_main.cuda_stream)
    cases = [pair(synth, "g0", 257, 390, lose=True), pair(synth, "g1", 40, 391), pair(synth, "g2", 100, 392, d=-2)]

    def reset():
        for s, c in enumerate(cases):
            rig.arm(s, c, mark=(s, 2 * s, 100 * s, 0))
        rig.stage()
    rows = ("feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags", "right_ok")
    dump = lambda: [rig.results()[k].tobytes() for k in sorted(rig.out) if k not in rows + ("right_xy",)] + \
        [rig.results()[k][s, :int(rig.results()["n_feat"][s])].tobytes() for s in range(3) for k in rows] + \
        [b for s in range(3) for b in _state_bytes(rig.state(s), rig.trk.get_ids(s))]
    reset(); rig.enqueue_init(60); torch.cuda.synchronize()
    eager = dump()
    assert rig.results()["report"][:, 0].tolist() == [0, api.Tracker.INIT_RETRY, 0]
    reset()
    g = api.StepGraph.record(s_main.cuda_stream, [s_side.cuda_stream], lambda: rig.enqueue_init(60))
    assert g.node_count() >= rig.trk.init_launches()
    assert (rig.results()["report"] == 0).all() and rig.trk.get_frame(0)["frozen"] == 1, "recording an init must not run it"
    for _ in range(2):
        g.launch(s_main.cuda_stream); torch.cuda.synchronize()
        assert dump() == eager
        reset()
