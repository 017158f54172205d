"""The multi-stream tracker (csrc/tracker.hip) on the hand-made states of tests/tracker_cases.py, in the lock-step form of
tests/test_gpu_tracker.py: each stream's state is downloaded, tests/tracker_ref.py computes the expected step from THAT state, and the device's
result is compared by check_step() below — bytes everywhere, class for non-finite start points (the hosts' NaN carries a sign bit the device's
does not), and the optimiser's pose, flags and inlier count at CheckedBackend.pose_only's bar.  tests/test_tracker_cases.py proves on the CPU
that every case reaches its path and that its inlier flags sit a factor 4 away from the chi2 threshold, so the budgeted soft rule of
CheckedBackend must never be needed here: every test asserts that.  check_step() itself is rehearsed on the CPU there, against stand-ins with
one deliberate fault each.

Figures measured on an MI355X are printed by each test (pytest -s); see DESIGN.md §3.20."""
import ctypes as C

import numpy as np
import pytest

import tracker_cases as TC
import tracker_ref as TR
from oracle_backend import CheckedBackend, OracleBackend

FILL = 0xA5
REC_KEYS = ("n_inliers", "n_features", "status", "frame_id", "needs_host")


class _DeviceResult:
    def pose_only(self, pose, p3, obs, Kt, pre=0):
        return self.result


def new_checker(chain, oracle):
    return CheckedBackend(_DeviceResult(), OracleBackend(oracle, None, None, chain))


def same_bits_or_class(a, b):
    """finite entries by bytes, NaN with NaN, inf with inf of the same sign"""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    fin = np.isfinite(b)
    return (a.shape == b.shape and np.array_equal(np.isfinite(a), fin) and a[fin].tobytes() == b[fin].tobytes()
            and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[np.isinf(b)], b[np.isinf(b)]))


def check_step(chain, oracle, K, good, bad, pre, prev_img, cur_img, dev, chk, tag):
    """one stream's step: dev = {"p0", "p1", "nxt", "lk_st" (debug_last_step), "post" (get_frame(image=True) after the step), "rec" (its record)}
    against the reference's step from `pre`.  The assertions of tests/test_gpu_tracker.py::_run, plus the stored image.  -> (expected, debug)"""
    post, rec = dev["post"], dev["rec"]
    _, _, e = TR.step(chain, oracle, K, pre, prev_img, cur_img, good, bad)
    assert same_bits_or_class(dev["p0"], e["p0"]) and same_bits_or_class(dev["p1"], e["p1"]), tag + ": LK start points are not the host's bits"
    lk = e["lk_status"]
    assert np.array_equal(dev["lk_st"], lk) and dev["nxt"][lk].tobytes() == e["nxt"][lk].tobytes(), tag + ": LK status / tracks"
    assert post["xy"].tobytes() == e["xy"].tobytes(), tag + ": current feature table"
    assert len(post["lm"]) == len(e["po"]), tag + ": current feature count"
    d_outl = np.array([post["lm"][j] < 0 for j in range(len(e["po"])) if e["po"][j] >= 0], bool)
    pose = np.array(rec["pose7"], float)
    if np.dot(pose[:4], e["pose"][:4]) < 0:              # the record's quaternion has w >= 0 (p7_of), the optimiser's own need not: q and -q are one
        pose[:4] = -pose[:4]                             # rotation, and beyond 90 degrees the two conventions part.  (The record's sign is checked
    chk.h.result = (pose, d_outl, int(rec["n_inliers"]))  # bit for bit below.)
    chk.pose_only(e["pose0"], e["p3"], e["obs"], K)                      # rtol = atol = 1e-6, flags and count equal
    assert not getattr(chk, "soft", {}), tag + ": the soft rule was needed although every flag of these cases has a factor 4 of margin"
    new, r2 = TR.finish(chain, pre, e["xy"], e["lm"], e["po"], np.array(rec["pose7"], float), d_outl, int(rec["n_inliers"]), good, bad)
    assert np.array_equal(post["lm"], new["lm"]) and np.array_equal(post["lm_outlier"], new["lm_outlier"]), tag + ": landmark flags"
    assert np.array_equal(post["outlier_list"], new["outlier_list"]), tag + ": outlier-landmark list"
    assert tuple(int(rec[k]) for k in ("status", "needs_host", "frame_id", "n_features")) == \
           (r2["status"], r2["needs_host"], r2["frame_id"], r2["n_features"]), tag + ": record"
    assert post["frozen"] == r2["needs_host"] and post["next_frame_id"] == pre["next_frame_id"] + 1 and post["status"] == r2["status"], tag + ": state"
    assert post["kf_every"] == pre["kf_every"] and post["ref_frame_id"] == pre["ref_frame_id"] and post["ref_pose"].tobytes() == pre["ref_pose"].tobytes()
    assert post["lm_pos"].tobytes() == pre["lm_pos"].tobytes(), tag + ": landmark positions"
    Tref = chain.T_of(pre["ref_pose"])
    assert chain.p7_of(chain.mm(post["last_rel"], Tref)).tobytes() == np.array(rec["pose7"], float).tobytes(), tag + ": record pose vs rel"
    assert chain.mm(post["last_rel"], chain.T_inv(pre["last_rel"])).tobytes() == post["rel_motion"].tobytes(), tag + ": relative motion"
    assert np.array_equal(post["image"], cur_img), tag + ": the stored image is not the step's new image"
    return r2, e


# ---------------------------------------------------------------------------------------------------------------- the device side
def device_images(torch, imgs, rows, cols, step, stride, offset=0):
    """images (None = a stream without one) at `offset + s * stride`, rows `step` apart, everything else FILL -> (tensor, address of image 0)"""
    buf = np.full(offset + len(imgs) * stride + 64, FILL, np.uint8)
    for s, im in enumerate(imgs):
        if im is not None:
            assert im.shape == (rows, cols)
            for r in range(rows):
                o = offset + s * stride + r * step
                buf[o:o + cols] = im[r]
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + offset


def state_bytes(st):
    return [np.asarray(st[k]).tobytes() for k in sorted(st)]


class Handle:
    """one api.Tracker with hand-made states; step() runs one step_batch and checks every stream against the reference"""

    def __init__(self, api, pkg, oracle, cases, cap, good=10, bad=4, rows=120, cols=160, lm_cap=None, layout=None):
        import torch
        self.api, self.chain, self.oracle, self.torch = api, pkg.chain, oracle, torch
        self.cases, self.S, self.rows, self.cols, self.good, self.bad = cases, len(cases), rows, cols, good, bad
        self.K = TC.K_of(rows, cols)
        self.layout = layout or (cols, rows * cols, 0)
        self.trk = api.Tracker(self.S, rows, cols, cap, lm_cap or cap, self.K, good, bad)
        self.chk = new_checker(pkg.chain, oracle)
        self.d_res = torch.zeros(self.S * 80, dtype=torch.uint8, device="cuda")
        for s, c in enumerate(cases):
            if c is not None:
                self.trk.set_frame(s, c["st"], image=c["prev"])

    def results(self):
        return self.d_res.cpu().numpy().view(self.api.TRACKER_RESULT_DTYPE)

    def step(self, curs=None, check=True):
        """curs: the new image of every stream (default: each case's "cur") -> {stream: dev dict of check_step + "exp" record}"""
        trk, torch = self.trk, self.torch
        curs = curs or [c["cur"] if c is not None else None for c in self.cases]
        pre = [trk.get_frame(s, image=self.cases[s] is not None) for s in range(self.S)]
        res0 = self.results().copy()
        step, stride, offset = self.layout
        keep, d_left = device_images(torch, curs, self.rows, self.cols, step, stride, offset)
        trk.step_batch(d_left, step, stride, self.d_res.data_ptr())
        torch.cuda.synchronize()
        res, out = self.results(), {}
        for s in range(self.S):
            tag = f"stream {s} ({self.cases[s]['name'] if self.cases[s] else 'never set'})"
            post = trk.get_frame(s, image=self.cases[s] is not None)
            if pre[s]["frozen"]:
                assert state_bytes(post) == state_bytes(pre[s]) and res[s].tobytes() == res0[s].tobytes(), tag + ": a frozen stream changed"
                assert trk.debug_last_step(s)[0].shape[0] == 0
                continue
            p0, p1, nxt, lk_st = trk.debug_last_step(s)
            out[s] = {"p0": p0, "p1": p1, "nxt": nxt, "lk_st": lk_st, "post": post, "rec": res[s].copy(), "pre": pre[s]}
            if check:
                out[s]["exp"], out[s]["dbg"] = check_step(self.chain, self.oracle, self.K, self.good, self.bad, pre[s], pre[s]["image"], curs[s],
                                                          out[s], self.chk, tag)
        del keep
        return out

    def worst(self):
        return self.chk.dev.get("pose_only_abs", 0.0)


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.gpu
def test_se3_branches_two_steps(api, pkg, synth, oracle):
    """every branch of se3_p7_of, the w < 0 flip, se3_T_of on -q and 3.7 q, translations of 1e3 - 1e4 m; the second step starts from the
    rel_motion and last_rel the first one's tail wrote"""
    cases = TC.se3_cases(pkg.chain, synth)
    h = Handle(api, pkg, oracle, cases, cap=256)
    seen, flips = set(), 0
    for k in range(2):
        out = h.step()
        assert len(out) == len(cases), f"step {k}: a stream froze"
        for s, d in out.items():
            for T in (TC.predicted_Tcw(pkg.chain, d["pre"]), pkg.chain.T_of(d["rec"]["pose7"])):
                b, f = TC.branch_of(T[:3, :3]); seen.add(b); flips += f
            assert d["rec"]["status"] == pkg.chain.TRACKING_GOOD and d["rec"]["n_inliers"] >= 20
    assert seen == {0, 1, 2, 3} and flips >= 1
    print(f"SE3 branches: {len(cases)} streams x 2 steps, branches {sorted(seen)}, {flips} sign flips, largest pose deviation {h.worst():.2e}")


LAYOUTS = [("odd_cols_odd_stride", 3, 118, 157, 161, 118 * 161 + 3, 0),          # byte path; stream 1 and 2 start on odd addresses
           ("pitch_dwords", 2, 120, 160, 164, 120 * 164 + 8, 0),                  # dword path with a row pitch
           ("pitch_base_plus_1", 2, 120, 160, 164, 120 * 164 + 8, 1),             # the same from d_left + 1: byte path
           ("rows_117", 2, 117, 160, 160, 117 * 160, 0)]                          # the last copy block holds one row


@pytest.mark.gpu
@pytest.mark.parametrize("name,S,rows,cols,step,stride,offset", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_image_layouts_two_steps(api, pkg, synth, oracle, name, S, rows, cols, step, stride, offset):
    """k_trk_head's two copy paths: padding and gaps hold 0xA5, the stored copy equals the unpadded image after each step (check_step), and the
    second step tracks FROM that copy and its pyramid"""
    cases, third = TC.layout_cases(pkg.chain, synth, name, S, rows, cols)
    h = Handle(api, pkg, oracle, cases, cap=64, rows=rows, cols=cols, layout=(step, stride, offset))
    out = h.step()
    out2 = h.step(third)
    assert len(out) == len(out2) == S and all(d["rec"]["n_features"] >= 20 for d in out2.values())
    print(f"image layout {name}: {S} streams x 2 steps, largest pose deviation {h.worst():.2e}")


@pytest.mark.gpu
def test_image_step_through_the_c_abi(api, pkg, synth, oracle):
    """myslam_tracker_set_frame / _get_frame with image_step = cols + 9: the step that follows tracks as from the contiguous image, get_frame
    leaves the caller's padding alone"""
    rows, cols, pitch = 118, 157, 157 + 9
    c = TC.abi_case(pkg.chain, synth)
    h = Handle(api, pkg, oracle, [c], cap=64, rows=rows, cols=cols)
    st = c["st"]
    padded = np.full((rows, pitch), FILL, np.uint8); padded[:, :cols] = c["prev"]
    xy = np.ascontiguousarray(st["xy"], np.float32); lm = np.ascontiguousarray(st["lm"], np.int32)
    pos = np.ascontiguousarray(st["lm_pos"]); fl = np.ascontiguousarray(st["lm_outlier"], np.uint8)
    ref = np.ascontiguousarray(st["ref_pose"]); rel = np.ascontiguousarray(st["last_rel"]); mot = np.ascontiguousarray(st["rel_motion"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = api.lib()
    h.trk.set_frame(0, st, image=np.zeros((rows, cols), np.uint8))          # what the pitched call has to replace
    assert L.myslam_tracker_set_frame(h.trk._h, 0, p(xy), p(lm), len(xy), p(pos), p(fl), len(pos), p(ref), st["ref_frame_id"], p(rel), p(mot),
                                      st["next_frame_id"], st["status"], st["kf_every"], p(padded), pitch) == api.OK

    def download():
        got = np.full((rows, pitch), FILL, np.uint8)
        assert L.myslam_tracker_get_frame(h.trk._h, 0, *([None] * 16), p(got), pitch) == api.OK
        return got
    assert np.array_equal(download(), padded)
    out = h.step()                                                            # check_step: against the reference FROM the contiguous image
    assert out[0]["rec"]["n_features"] >= 20 and np.array_equal(out[0]["pre"]["image"], c["prev"])
    got = download()
    assert np.array_equal(got[:, :cols], c["cur"]) and (got[:, cols:] == FILL).all()


@pytest.mark.gpu
def test_counts_on_the_round_boundaries(api, pkg, synth, oracle):
    """k_trk_compact / k_trk_tail: n_feat 0, 1, 63 .. 65, 255 .. 257, 511 .. 513 and cap, every seventh feature lost (outside, NaN, no
    landmark), flagged landmarks and shared landmarks in every stream — twelve streams in one call"""
    cases = [TC.count_case(pkg.chain, synth, n, "mixed", seed=k) for k, n in enumerate(TC.COUNTS)]
    h = Handle(api, pkg, oracle, cases, cap=1024)
    out = h.step()
    assert [len(out[s]["pre"]["lm"]) for s in range(12)] == TC.COUNTS
    kept = [int(out[s]["rec"]["n_features"]) for s in range(12)]
    assert all(0 <= TC.COUNTS[s] - len(cases[s]["lost"]) - kept[s] <= 2 for s in range(12)), kept          # (LK may lose one more on a flat patch)
    print(f"counts: kept {kept} of {TC.COUNTS}, largest pose deviation {h.worst():.2e}")


@pytest.mark.gpu
def test_keep_patterns_around_a_frozen_stream(api, pkg, synth, oracle):
    """all lost; only the last kept (its slot is 0 after 256 / 512 lost ones); a never-set stream between active ones stays untouched"""
    cases = TC.keep_pattern_cases(pkg.chain, synth)
    h = Handle(api, pkg, oracle, cases, cap=1024)
    h.d_res.fill_(0x5C)
    out = h.step()
    assert sorted(out) == [0, 2, 3, 4, 5] and [int(out[s]["rec"]["n_features"]) for s in (0, 2, 3, 4)] == [0, 1, 1, 0]
    assert h.results()[1].tobytes() == bytes([0x5C]) * 80 and h.trk.get_frame(1)["frozen"] == 1
    assert all(out[s]["rec"]["status"] == pkg.chain.LOST and out[s]["post"]["frozen"] == 1 for s in (0, 2, 3, 4))
    assert len(h.step()) == 1                                                 # the LOST streams are frozen now: the next step leaves them alone


BLOCKS = [("S64_cap256_64_threads", 64, 256, 40, 250), ("S64_cap512_128_threads", 64, 512, 40, 250)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,S,cap,lo,hi", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_pose_only_block_sizes_of_large_banks(api, pkg, synth, oracle, name, S, cap, lo, hi):
    """pose_only_launch's forms from S = 64 on, against the reference; stream 5 against the same state alone (S = 1: 256-thread blocks) at the
    bar of test_gpu_tracker.py::test_stream_results_do_not_depend_on_the_bank"""
    cases = TC.bank_cases(pkg.chain, synth, S, lo, hi)
    h = Handle(api, pkg, oracle, cases, cap=cap)
    out = h.step()
    assert len(out) == S and out[3]["rec"]["n_features"] == 0
    one = Handle(api, pkg, oracle, [cases[5]], cap=cap).step(check=False)[0]
    a, b = out[5], one
    assert a["p1"].tobytes() == b["p1"].tobytes() and np.array_equal(a["lk_st"], b["lk_st"]) and a["nxt"][a["lk_st"]].tobytes() == b["nxt"][b["lk_st"]].tobytes()
    dev = float(np.abs(a["rec"]["pose7"] - b["rec"]["pose7"]).max())
    assert np.allclose(a["rec"]["pose7"], b["rec"]["pose7"], rtol=1e-8, atol=1e-9), dev
    assert all(a["rec"][f] == b["rec"][f] for f in REC_KEYS)
    print(f"block size {name}: largest pose deviation from the reference {h.worst():.2e}, stream 5 in the bank against alone {dev:.2e}")


@pytest.mark.gpu
def test_pose_only_block_size_of_cap_4096(api, pkg, synth, oracle):
    """512-thread blocks: S = 2, cap 4096 with 4096 and 3000 features"""
    cases = TC.cap4096_cases(pkg.chain, synth)
    h = Handle(api, pkg, oracle, cases, cap=4096)
    out = h.step()
    assert [int(out[s]["rec"]["n_features"]) for s in (0, 1)] == [4096, 3000]
    print(f"block size S2_cap4096_512_threads: largest pose deviation from the reference {h.worst():.2e}")


def _threshold_state(pkg, synth, oracle):
    c = TC.threshold_case(pkg.chain, synth)
    n = TR.step(pkg.chain, oracle, c["K"], c["st"], c["prev"], c["cur"], 0, 0)[1]["n_inliers"]
    return c, n


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["good", "bad", "lost"])
def test_status_thresholds_and_key_frame_rule(api, pkg, synth, oracle, which):
    """n = the reference's inlier count: (good, bad) = (n - 1, 0) -> GOOD, (n, n - 1) -> BAD, (n + 5, n) -> LOST: `>` on both thresholds;
    frame id % kf_every at 0, at negative ids and with kf_every 1"""
    chain = pkg.chain
    c, n = _threshold_state(pkg, synth, oracle)
    assert n >= 20
    good, bad, status = {"good": (n - 1, 0, chain.TRACKING_GOOD), "bad": (n, n - 1, chain.TRACKING_BAD), "lost": (n + 5, n, chain.LOST)}[which]
    cases = [dict(c, name=f"kf{kfe}_id{fid}", st=dict(c["st"], kf_every=kfe, next_frame_id=fid, ref_frame_id=fid - 5)) for kfe, fid in TC.KF_IDS]
    h = Handle(api, pkg, oracle, cases, cap=64, good=good, bad=bad)
    out = h.step()
    for s, (kfe, fid) in enumerate(TC.KF_IDS):
        rec = out[s]["rec"]
        want = status == chain.LOST or (status == chain.TRACKING_BAD if kfe == 0 else fid % kfe == 0)
        assert rec["n_inliers"] == n and rec["status"] == status and rec["needs_host"] == int(want) == out[s]["post"]["frozen"], (which, kfe, fid)
        assert out[s]["exp"]["needs_host"] == int(want)
    print(f"thresholds ({which}): n_inliers {n}, (good, bad) = ({good}, {bad}), needs_host {[int(out[s]['rec']['needs_host']) for s in range(7)]}")


@pytest.mark.gpu
def test_fresh_landmark_rule_at_2_and_3(api, pkg, synth, oracle):
    cases = TC.fresh_cases(pkg.chain, synth)
    h = Handle(api, pkg, oracle, cases, cap=64)
    out = h.step()
    l2, l3 = out[0]["post"]["outlier_list"].tolist(), out[1]["post"]["outlier_list"].tolist()
    assert len(l2) >= 4 and l2.count(21) == 2 and l3 == [] and out[1]["post"]["lm_outlier"].sum() == 0
    assert out[0]["post"]["lm_outlier"].sum() == len(set(l2)) and (out[1]["post"]["lm"] < 0).sum() == len(l2)
    print(f"fresh rule: list at 2: {l2}, at 3: {l3}")


@pytest.mark.gpu
def test_non_finite_predictions(api, pkg, synth, oracle):
    """landmarks at the camera centre, in its plane, behind it and beyond the float range: start points NaN / inf / mirrored / inf as the hosts
    compute them, LK loses the non-finite ones, the rest of the step equals the reference; the streams beside it are what they are without it"""
    chain = pkg.chain
    bad_case = TC.nonfinite_case(chain, synth)
    a, b = TC.beside_cases(chain, synth)
    h3 = Handle(api, pkg, oracle, [a, bad_case, b], cap=128)
    out = h3.step()
    p1, lk = out[1]["p1"], out[1]["lk_st"]
    for i, kind in bad_case["kinds"].items():
        u, v = p1[i]
        assert {"nan": np.isnan(u) and np.isnan(v), "inf": np.isinf(u), "mirrored": np.isfinite(u) and np.isfinite(v), "overflow": np.isinf(u) and np.isfinite(v)}[kind], (i, kind, u, v)
        assert kind == "mirrored" or not lk[i], (i, kind)
    assert out[1]["rec"]["n_features"] >= 40 and np.isfinite(out[1]["rec"]["pose7"]).all()
    h2 = Handle(api, pkg, oracle, [a, b], cap=128)
    out2 = h2.step(check=False)
    for s3, s2 in ((0, 0), (2, 1)):
        assert out[s3]["rec"].tobytes() == out2[s2]["rec"].tobytes() and state_bytes(out[s3]["post"]) == state_bytes(out2[s2]["post"])
        assert all(out[s3][k].tobytes() == out2[s2][k].tobytes() for k in ("p0", "p1", "nxt", "lk_st"))
    print(f"non-finite predictions: {int((~lk).sum())} lost of {len(lk)}, kept {int(out[1]['rec']['n_features'])}, largest pose deviation {h3.worst():.2e}")


@pytest.mark.gpu
def test_argument_checks_leave_state_and_results_alone(api, pkg, synth):
    import torch
    c = TC.make(pkg.chain, synth, "args", n=30, seed=95)
    trk = api.Tracker(2, 120, 160, 64, 64, c["K"], 10, 4)
    with pytest.raises(api.MyslamError) as e:
        trk.set_frame(1, c["st"])                                             # no image on a never-set stream
    assert e.value.code == api.ERR_INVALID and trk.get_frame(1)["frozen"] == 1
    trk.set_frame(0, c["st"], image=c["prev"])
    before = state_bytes(trk.get_frame(0, image=True))
    for bad_lm in (len(c["st"]["lm_pos"]), -2):
        st = dict(c["st"], lm=c["st"]["lm"].copy(), next_frame_id=99); st["lm"][7] = bad_lm
        with pytest.raises(api.MyslamError) as e:
            trk.set_frame(0, st, image=c["cur"][::-1])
        assert e.value.code == api.ERR_INVALID and state_bytes(trk.get_frame(0, image=True)) == before
    keep, d_left = device_images(torch, [c["cur"], c["cur"]], 120, 160, 160, 120 * 160)
    d_res = torch.full((2 * 80,), 0x5C, dtype=torch.uint8, device="cuda")
    for step, stride in ((159, 120 * 160), (160, 119 * 160 + 159), (164, 119 * 164 + 159)):
        with pytest.raises(api.MyslamError) as e:
            trk.step_batch(d_left, step, stride, d_res.data_ptr())
        assert e.value.code == api.ERR_INVALID
    torch.cuda.synchronize()
    assert (d_res.cpu().numpy() == 0x5C).all() and state_bytes(trk.get_frame(0, image=True)) == before
