"""The hand-made tracker states of tests/tracker_cases.py hold their conditions on the reference alone (tests/tracker_ref.py with the oracle's LK
and pose-only): every case reaches the path it is named after, tracks at least 20 features where it is meant to, and every flag of the pose-only
problem sits a factor 4 away from the chi2 threshold, so that the device (tests/test_gpu_tracker_edges.py) cannot legitimately differ in a flag.
A case that stops exercising its path fails HERE.  The second half rehearses that file's comparison helper on the CPU: a stand-in for the
device's result, built from the reference with one deliberate fault, must be rejected.  CPU only."""
import numpy as np
import pytest

import tracker_cases as TC
import tracker_ref as TR
from test_gpu_tracker_edges import check_step, new_checker

GOOD, BAD = 10, 4


def _sq_errors(chain, K, dbg):
    T = chain.T_of(dbg["pose"])
    uv = np.array([TR.world2pixel(chain, K, p, T) for p in dbg["p3"]]).reshape(-1, 2)
    return ((uv - dbg["obs"]) ** 2).sum(1)


def _margins(chain, K, dbg, tag):
    e2 = _sq_errors(chain, K, dbg)
    o = dbg["outlier"]
    assert (e2[~o] < TC.CHI2 / 4).all(), (tag, "an inlier within a factor 4 of the threshold", float(e2[~o].max()))
    assert (e2[o] > 4 * TC.CHI2).all(), (tag, "an outlier within a factor 4 of the threshold", float(e2[o].min()))
    return e2


def _run(chain, oracle, case, curs=None, good=GOOD, bad=BAD, min_tracked=20):
    """the reference's steps of one case (the second from the first one's state and image), margins asserted -> [(state, record, debug)]"""
    st, prev, out = case["st"], case["prev"], []
    for k, cur in enumerate(curs or [case["cur"]]):
        new, rec, dbg = TR.step(chain, oracle, case["K"], st, prev, cur, good, bad)
        tag = f"{case['name']} step {k}"
        _margins(chain, case["K"], dbg, tag)
        assert rec["n_features"] >= min_tracked and rec["n_inliers"] >= min_tracked, (tag, rec)
        if k == 0:                                       # every intended outlier that reached the optimiser is one
            rows = {int(i): dbg["po"][j] for j, i in enumerate(np.flatnonzero(_kept(st, dbg)))}
            hit = [rows[i] for i in case["outliers"] if i in rows and rows[i] >= 0]
            assert dbg["outlier"][hit].all() and dbg["outlier"].sum() == len(hit), (tag, "outliers", hit, np.flatnonzero(dbg["outlier"]))
            case["n_outliers_hit"] = len(hit)
        out.append((new, rec, dbg))
        st, prev = new, cur
    return out


def _kept(st, dbg):
    return dbg["lk_status"] & (np.asarray(st["lm"]) >= 0)


def test_se3_cases_take_every_branch(pkg, synth, oracle):
    chain = pkg.chain
    seen, flips, big = set(), 0, 0
    for c in TC.se3_cases(chain, synth):
        steps = _run(chain, oracle, c, [c["cur"], c["cur"]])
        st = c["st"]
        for (new, rec, dbg), pre in zip(steps, [st, steps[0][0]]):
            assert rec["status"] == chain.TRACKING_GOOD and not rec["needs_host"]
            for T in (TC.predicted_Tcw(chain, pre), chain.mm(new["last_rel"], chain.T_of(pre["ref_pose"]))):
                R = T[:3, :3]
                t = R[0, 0] + R[1, 1] + R[2, 2]                                  # recomputed here, not taken from the builder
                d = np.diag(R)
                b = 0 if t > 0 else (1 if d[0] > d[1] and d[0] > d[2] else (2 if d[1] > d[2] else 3))
                w = [1.0, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]][b]
                assert (b, w < 0) == TC.branch_of(R)
                seen.add(b); flips += w < 0
                big += 1e3 <= np.abs(T[:3, 3]).max() <= 2e4
        assert c["n_outliers_hit"] == 3
        q = st["ref_pose"][:4]
        assert c["name"].endswith("negated") == (q[3] < 0) and c["name"].endswith(("scaled", "reversed")) == (abs(np.sqrt((q * q).sum()) - 3.7) < 1e-12)
    assert seen == {0, 1, 2, 3} and flips >= 1 and big == 7 * 4, (seen, flips, big)
    moved = [c for c in TC.se3_cases(chain, synth) if not np.array_equal(c["st"]["rel_motion"], np.eye(4))]
    assert len(moved) == 2


@pytest.mark.parametrize("rows,cols", TC.SIZES)
def test_layout_cases_track_over_two_steps(pkg, synth, oracle, rows, cols):
    cases, third = TC.layout_cases(pkg.chain, synth, "layout", 3, rows, cols)
    for c, t in zip(cases, third):
        steps = _run(pkg.chain, oracle, c, [c["cur"], t])
        assert c["n_outliers_hit"] == 3 and not steps[0][1]["needs_host"]
        assert not np.array_equal(c["cur"], t) and steps[1][2]["lk_status"].sum() >= 20
    _run(pkg.chain, oracle, TC.abi_case(pkg.chain, synth))


def test_count_cases_hit_the_round_boundaries(pkg, synth, oracle):
    chain = pkg.chain
    assert TC.COUNTS == [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024]
    for k, n in enumerate(TC.COUNTS):
        c = TC.count_case(chain, synth, n, "mixed", seed=k)
        st = c["st"]
        new, rec, dbg = _run(chain, oracle, c, min_tracked=0)[0]
        kept = _kept(st, dbg)
        gone = set(np.flatnonzero(~kept).tolist())          # (LK may also lose a feature on a flat patch: the reference decides, a few at most)
        assert len(st["lm"]) == n and gone >= set(c["lost"]) and len(gone) <= len(c["lost"]) + 2, c["name"]
        for base in range(0, n, 256):                    # a lost and a kept feature in every round where n allows
            r = kept[base:base + 256]
            assert len(r) < 4 or (r.any() and not r.all()), (c["name"], base)
        if n >= 8:
            lm = st["lm"][kept]
            flagged = st["lm_outlier"][lm] == 1
            assert flagged.any() and (dbg["po"][flagged] == -1).all() and (dbg["po"][~flagged] >= 0).all()
            assert len(set(lm[~flagged].tolist())) < (~flagged).sum() and len(set(lm[flagged].tolist())) < flagged.sum(), "shared landmarks"
        if n >= 63:
            lost_by = {kind: 0 for kind in TC.LOST_KINDS}
            for i in c["lost"]:
                lost_by["no_landmark" if st["lm"][i] < 0 else ("nan" if np.isnan(st["xy"][i, 0]) else "outside")] += 1
            assert min(lost_by.values()) >= 2, lost_by
    for c in TC.keep_pattern_cases(chain, synth):
        if c is None:
            continue
        new, rec, dbg = _run(chain, oracle, c, min_tracked=0)[0]
        kept = np.flatnonzero(_kept(c["st"], dbg)).tolist()
        n = len(c["st"]["lm"])
        want = {"all_lost": [], "last_kept": [n - 1], "mixed": [i for i in range(n) if i % 7 != 3]}[c["name"].split("_", 1)[1]]
        assert set(kept) <= set(want) and len(kept) >= len(want) - 2 and (len(want) > 1 or kept == want) and (c["st"]["lm_outlier"] == 1).any() and len(set(c["st"]["lm"].tolist())) < n, c["name"]
        assert rec["status"] == (chain.TRACKING_GOOD if len(kept) > 10 else chain.LOST)


def test_bank_and_large_cap_cases(pkg, synth, oracle):
    cases = TC.bank_cases(pkg.chain, synth, 64, 40, 250)
    ns = [len(c["st"]["lm"]) for c in cases]
    assert min(n for n in ns if n) == 40 and max(ns) == 250 and ns[3] == 0 and len(set(ns)) > 30
    for c in cases:
        _run(pkg.chain, oracle, c, min_tracked=min(20, len(c["st"]["lm"])))
    big = TC.cap4096_cases(pkg.chain, synth)
    assert [len(c["st"]["lm"]) for c in big] == [4096, 3000]
    for c in big:
        rec = _run(pkg.chain, oracle, c)[0][1]
        assert rec["n_features"] == len(c["st"]["lm"]) and c["n_outliers_hit"] == 3


def test_threshold_and_fresh_cases(pkg, synth, oracle):
    chain = pkg.chain
    c = TC.threshold_case(chain, synth)
    n = _run(chain, oracle, c)[0][1]["n_inliers"]
    assert n >= 20 and c["n_outliers_hit"] == 3
    for good, bad, status in ((n - 1, 0, chain.TRACKING_GOOD), (n, n - 1, chain.TRACKING_BAD), (n + 5, n, chain.LOST)):
        assert _run(chain, oracle, c, good=good, bad=bad)[0][1]["status"] == status
    f2, f3 = TC.fresh_cases(chain, synth)
    for c, d in ((f2, 2), (f3, 3)):
        new, rec, dbg = _run(chain, oracle, c)[0]
        assert c["st"]["next_frame_id"] - c["st"]["ref_frame_id"] == d and dbg["outlier"].sum() >= 3 and c["n_outliers_hit"] == 5
        lst = new["outlier_list"].tolist()
        assert (lst.count(21) == 2 and len(lst) == 5 and new["lm_outlier"].sum() == 4) if d == 2 else (lst == [] and new["lm_outlier"].sum() == 0)
        assert (new["lm"] < 0).sum() == 5


def test_nonfinite_case_classes(pkg, synth, oracle):
    chain = pkg.chain
    c = TC.nonfinite_case(chain, synth)
    assert np.array_equal(c["st"]["ref_pose"], chain.IDENT) and np.array_equal(TC.predicted_Tcw(chain, c["st"]), np.eye(4))
    with np.errstate(all="ignore"):
        new, rec, dbg = _run(chain, oracle, c)[0]
    kinds = sorted(set(c["kinds"].values()))
    assert kinds == ["inf", "mirrored", "nan", "overflow"]
    for i, kind in c["kinds"].items():
        u, v = dbg["p1"][i]
        ok = {"nan": np.isnan(u) and np.isnan(v), "inf": np.isinf(u), "mirrored": np.isfinite(u) and np.isfinite(v) and c["st"]["lm_pos"][i][2] < 0,
              "overflow": np.isinf(u) and np.isfinite(v)}[kind]
        assert ok, (i, kind, u, v)
        assert not dbg["lk_status"][i] if kind != "mirrored" else dbg["lk_status"][i], (i, kind)
    assert [tuple(c["st"]["lm_pos"][40 + 3 * k]) for k in range(4)] == [p for _, p in TC.BAD_LANDMARKS]
    for b in TC.beside_cases(chain, synth):
        _run(chain, oracle, b)


# ---------------------------------------------------------------------------------------- the comparison helper can fail (CPU rehearsal)
def _stand_in(chain, oracle, case, good=GOOD, bad=BAD):
    """what a faultless device would hand to check_step, built from the reference"""
    new, rec, dbg = TR.step(chain, oracle, case["K"], case["st"], case["prev"], case["cur"], good, bad)
    post = dict(new, image=case["cur"].copy())
    dev = {"p0": dbg["p0"].copy(), "p1": dbg["p1"].copy(), "nxt": dbg["nxt"].copy(), "lk_st": dbg["lk_status"].copy(), "post": post, "rec": dict(rec)}
    return dev, dbg


def _check(chain, oracle, case, dev, good=GOOD, bad=BAD):
    return check_step(chain, oracle, case["K"], good, bad, case["st"], case["prev"], case["cur"], dev, new_checker(chain, oracle), case["name"])


def _swapped_R_to_q(R):
    """chain.R_to_q with the bodies of its second and third branch exchanged"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0) * 2; q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2; q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2; q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2; q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    return q if q[3] >= 0 else -q


def test_rehearsal_a_faultless_stand_in_passes(pkg, synth, oracle):
    for c in TC.se3_cases(pkg.chain, synth)[:2] + [TC.count_case(pkg.chain, synth, 257, "mixed", seed=7), TC.nonfinite_case(pkg.chain, synth)]:
        with np.errstate(all="ignore"):
            _check(pkg.chain, oracle, c, _stand_in(pkg.chain, oracle, c)[0])


def test_rehearsal_swapped_quaternion_branch_is_rejected(pkg, synth, oracle):
    chain = pkg.chain
    hit = 0
    for c in TC.se3_cases(chain, synth):
        dev, dbg = _stand_in(chain, oracle, c)
        T = chain.mm(dev["post"]["last_rel"], chain.T_of(c["st"]["ref_pose"]))
        if TC.branch_of(T[:3, :3])[0] not in (1, 2):
            continue
        dev["rec"]["pose7"] = np.concatenate([_swapped_R_to_q(T[:3, :3]), T[:3, 3]])
        with pytest.raises(AssertionError):
            _check(chain, oracle, c, dev)
        hit += 1
    assert hit >= 2
    # ... and a sign flip forgotten in the record's pose
    c = [c for c in TC.se3_cases(chain, synth) if c["name"] == "skew170_reversed"][0]
    dev, _ = _stand_in(chain, oracle, c)
    T = chain.mm(dev["post"]["last_rel"], chain.T_of(c["st"]["ref_pose"]))
    assert TC.branch_of(T[:3, :3])[1]
    dev["rec"]["pose7"][:4] *= -1
    with pytest.raises(AssertionError, match="record pose"):
        _check(chain, oracle, c, dev)


def test_rehearsal_dropped_image_row_is_rejected(pkg, synth, oracle):
    cases, _ = TC.layout_cases(pkg.chain, synth, "layout", 2, 117, 160)
    for c, row in zip(cases, (116, 0)):
        dev, _ = _stand_in(pkg.chain, oracle, c)
        dev["post"]["image"][row] = 0xA5
        with pytest.raises(AssertionError, match="stored image"):
            _check(pkg.chain, oracle, c, dev)


def test_rehearsal_off_by_one_rank_is_rejected(pkg, synth, oracle):
    """the features of the second round of 256 land one slot late"""
    chain = pkg.chain
    c = TC.count_case(chain, synth, 513, "mixed", seed=10)
    dev, dbg = _stand_in(chain, oracle, c)
    first = int(_kept(c["st"], dbg)[:256].sum())
    for key in ("xy", "lm"):
        a = dev["post"][key].copy()
        a[first + 1:] = dev["post"][key][first:-1]
        dev["post"][key] = a
    with pytest.raises(AssertionError):
        _check(chain, oracle, c, dev)
    # ... and a pose-only row off by one: the flag lands on the neighbouring feature
    c = TC.threshold_case(chain, synth)
    dev, dbg = _stand_in(chain, oracle, c)
    lm = dev["post"]["lm"]
    j = int(np.flatnonzero(lm < 0)[0])
    lm[j], lm[j + 1] = dbg["lm"][j], -1
    with pytest.raises(AssertionError):
        _check(chain, oracle, c, dev)


def test_rehearsal_status_rule_with_equality_is_rejected(pkg, synth, oracle):
    chain = pkg.chain
    c = TC.threshold_case(chain, synth)
    n = TR.step(chain, oracle, c["K"], c["st"], c["prev"], c["cur"], 0, 0)[1]["n_inliers"]
    for good, bad, wrong in ((n, n - 1, chain.TRACKING_GOOD), (n + 5, n, chain.TRACKING_BAD)):
        dev, _ = _stand_in(chain, oracle, c, good, bad)
        _check(chain, oracle, c, dev, good, bad)
        dev["rec"]["status"] = dev["post"]["status"] = wrong                    # `>=` for `>`
        with pytest.raises(AssertionError, match="record"):
            _check(chain, oracle, c, dev, good, bad)
