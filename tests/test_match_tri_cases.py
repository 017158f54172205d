"""The hand-made matcher and triangulation inputs of tests/match_tri_cases.py hold their conditions on the oracle alone: every Hamming case has the
closed-form answer it claims and reaches the position, distance or count it is named for; every case of the triangulation's gate ladder is classed
stable or unstable by nine evaluations of the oracle's general f64 entry, at least 99 % are stable, and each intrinsics set has stable cases on
both sides of both gates.  The second half feeds the comparison helpers of tests/test_gpu_match_edges.py stand-ins for the device — the oracle's
answer restated in numpy with ONE fault each — and every one must be rejected.  CPU only."""
import numpy as np
import pytest

import match_tri_cases as MC
from test_gpu_match_edges import INTRINSICS, check_hamming, check_tri


def _oracle_all(oracle, case):
    q, nq, t, nt, ei, ed = case
    cap = q.shape[1]
    gi = np.full_like(ei, MC.SENTINEL); gd = np.full_like(ed, MC.SENTINEL)
    for b in range(len(nq)):
        n, m = MC.clamp(nq[b], cap), MC.clamp(nt[b], cap)
        gi[b, :n], gd[b, :n] = oracle.hamming_match(q[b, :n], t[b, :m])
    return gi, gd


@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in MC.HAMMING_BUILDERS.items()}


# ------------------------------------------------------------------------------------------------------------------------ Hamming cases
@pytest.mark.parametrize("builder", list(MC.HAMMING_BUILDERS))
def test_oracle_gives_the_closed_form(oracle, cases, builder):
    case = cases[builder]
    gi, gd = _oracle_all(oracle, case)
    assert np.array_equal(gi, case[4]) and np.array_equal(gd, case[5])
    check_hamming(oracle, case, gi, gd, builder)            # the helper accepts a faultless answer
    q, nq, t, nt = case[:4]
    assert q.shape[1] <= 192 and (np.clip(nq, 0, q.shape[1]) <= 40).all() and q.shape == t.shape and q.dtype == t.dtype == np.uint8


def test_suffix_ties_put_the_first_tied_row_everywhere(cases):
    q, nq, t, nt, ei, ed = cases["suffix_ties"]
    assert (nt == 161).all() and len(nt) == 161 and 161 == 5 * 32 + 1
    for s in range(161):
        n = nq[s]
        assert (t[s, s:161] == t[s, s]).all() and (ei[s, :n] == s).all() and ed[s, :n].max() <= 3 and ed[s, :n].min() == 0
        assert np.array_equal(MC.popcount(q[s, :n], t[s, s]), ed[s, :n])
        if s:
            assert MC.popcount(q[s, :n, None], t[s, None, :s]).min() >= 60        # the rows before it are far
    assert {33, 40} <= set(nq.tolist())                 # a second query tile with one row, and with eight


def test_pair_ties_are_the_listed_ones(cases):
    q, nq, t, nt, ei, ed = cases["pair_ties"]
    listed = [r for r, _ in MC.PAIR_TIES]
    for want in [(0, 1), (3, 4), (7, 8), (31, 32), (127, 128), (5, 37), (33, 161), (40, 130), (100, 128)]:
        assert want in listed
    assert sum(len(r) == 3 for r in listed) >= 3
    for b, (rows, n_t) in enumerate(MC.PAIR_TIES):
        assert nt[b] == n_t and max(rows) < n_t and list(rows) == sorted(rows)
        d = MC.popcount(q[b, :nq[b], None], t[b, None, :n_t])
        tied = np.zeros(n_t, bool); tied[list(rows)] = True
        assert (d[:, tied] == ed[b, :nq[b], None]).all() and (d[:, ~tied] > ed[b, :nq[b], None]).all()      # every other row strictly farther
        assert (ei[b, :nq[b]] == rows[0]).all()
    # the later row owned by group 0's next step while the earlier belongs to a higher group; b as the last row of a partial tail chunk
    grp = lambda r: (r // 32) % 4
    assert all(grp(a) > 0 and grp(b) == 0 and b // 32 >= 4 for a, b in [(40, 130), (100, 128)])
    assert any(rows[-1] == n_t - 1 and n_t % 32 for rows, n_t in MC.PAIR_TIES) and (33 // 32) % 4 == (161 // 32) % 4


def test_distance_ladder_reaches_every_distance(cases):
    q, nq, t, nt, ei, ed = cases["distance_ladder"]
    assert len(nq) == 258
    for m in range(257):
        d = MC.popcount(q[m, 0], t[m, :nt[m]])
        pos = ei[m, 0]
        assert nt[m] % 32 and d.min() == m == ed[m, 0] and (d == m).sum() == 1 and d[pos] == m, m
        if m < 256:
            assert (d[:pos] == m + 1).any(), m
        assert (ed[m, :nq[m]] == m).all() and (q[m, :nq[m]] == q[m, 0]).all()
        assert (MC.popcount(q[m, 0], t[m, nt[m]:]) == 0).all()                 # the rows the kernel must not see would win
    for m in (0, 1, 127, 128, 129, 255, 256):
        assert ed[m, 0] == m
    assert nt[256] == 1 and nt[257] == 70 and (MC.popcount(q[257, 0], t[257, :70]) == 256).all() and ei[257, 0] == 0
    assert len({int(ei[m, 0]) // 32 == (int(nt[m]) - 1) // 32 for m in range(256)}) == 2     # answers in the tail chunk and before it
    flipped = np.unpackbits(q[:256, 0, None, :] ^ t[:256, :37], axis=-1).reshape(-1, 256).sum(0)
    assert flipped.min() > 0                            # flipped bits over all 32 bytes


def test_count_edges_cover_the_listed_counts(cases):
    q, nq, t, nt, ei, ed = cases["count_edges"]
    cap = q.shape[1]
    edge = {cap + 1, 2 * cap, MC.I32_MAX, -1, MC.I32_MIN}
    assert edge <= set(nq.tolist()) and edge <= set(nt.tolist())
    assert any(0 < a <= cap and 0 < b <= cap for a, b in zip(nq, nt))
    for b in range(len(nq)):
        n = MC.clamp(nq[b], cap)
        assert (ei[b, n:] == MC.SENTINEL).all() and (ed[b, n:] == MC.SENTINEL).all()
        if nq[b] < 0:
            assert n == 0
        if nq[b] > cap:
            assert n == cap and (ei[b] != MC.SENTINEL).all()
        if nt[b] <= 0 and n:
            assert (ei[b, :n] == -1).all() and (ed[b, :n] == -1).all()
        if nt[b] > cap and n:
            assert ei[b, 0] == cap - 1 and ed[b, 0] == 0          # the last row a clamped count covers
    assert any(a > 0 and b < 0 for a, b in zip(nq, nt))


# ------------------------------------------------------------------------------------------------------------------------ gate ladder
@pytest.mark.parametrize("name", INTRINSICS)
def test_gate_ladder_is_stable_and_populates_both_sides(oracle, synth, name):
    L = MC.gate_ladder(oracle, synth, name)
    ref = L["ref"]
    n = len(ref["ok"])
    K5 = L["K5"]
    assert sorted(set(np.abs(L["disp"]).tolist()) - {0.0}) == [2.0 ** k for k in range(-7, 10)] and (L["disp"] < 0).sum() == (L["disp"] > 0).sum()
    assert {0.0, 30.0, -30.0} <= set(L["dy"].tolist())
    # the ladder is dense where the reference's own ratio crosses the gate: cases within 0.2 % of it on both sides
    near = np.abs(ref["ratio"] / MC.RATIO_GATE - 1) < 2e-3
    assert (near & (ref["ratio"] < MC.RATIO_GATE)).sum() > 100 and (near & (ref["ratio"] >= MC.RATIO_GATE)).sum() > 100
    xs = set(L["xl"].tolist())
    assert any(x < 0 for x in xs) and any(x > 9e3 for x in xs) and any(0 <= x <= 1240 for x in xs) and len(xs) == 10          # five left points, and one pixel beside each for disparity 0
    st = ref["stable"]
    assert st.mean() >= 0.99, (name, 1 - st.mean())
    z = ref["xyz"][:, 2]
    for side in (ref["ratio"] < MC.RATIO_GATE, ref["ratio"] >= MC.RATIO_GATE, z > 0, z < 0):
        assert (st & side).sum() >= 100, name
    assert (st & ref["ok"]).sum() >= 100 and (st & ~ref["ok"] & (z > 0)).sum() >= 100 and (st & (ref["ratio"] < MC.RATIO_GATE) & (z < 0)).sum() >= 100
    zero = L["disp"] == 0
    assert zero.sum() == 5 and not st[zero].any()       # disparity exactly 0: kept, and unstable as expected
    ok2 = oracle.triangulate_stereo(L["xl"], L["yl"], L["xr"], L["yr"], *K5)[1]
    assert np.array_equal(ok2[st], ref["ok"][st])       # the stereo entry decides as the general one does
    if name == "anisotropic_off_centre":
        assert K5[0] != K5[1] and K5[2] < 0 and K5[3] > MC.IMG_H
    print(f"\n{name}: {n} cases, {int((~st).sum())} unstable ({100 * (1 - st.mean()):.2f} %), ratio {ref['ratio'][st].min():.2e} .. {ref['ratio'][st].max():.2e}")


def test_baselines_and_crossings_differ_per_set(oracle, synth):
    K = MC.intrinsics(synth)
    assert K["baseline_5cm"][4] == 0.05 and K["baseline_5m"][4] == 5.0 and K["kitti00"][:4] == (synth.KITTI00["fx"], synth.KITTI00["fy"], synth.KITTI00["cx"], synth.KITTI00["cy"])
    c = {n: MC.crossing(oracle, K[n], MC.POSITIONS[0], 1.0, 1.0) for n in K}
    assert 3.0 < c["kitti00"] < 4.5                      # ~2.7e-3 per pixel of vertical offset
    assert c["baseline_5cm"] < 0.5 and c["baseline_5m"] > 8      # not a constant: found per set with the oracle
    for n in K:                                          # ... and it is the crossing
        poses = MC._poses(K[n][4])
        x, y = np.float32(MC.POSITIONS[0][0]), np.float32(MC.POSITIONS[0][1])
        r = [MC.solve(oracle, poses, MC.normalised(K[n], (x, y, x - np.float32(1), np.float64(y) + f * c[n])))[1] for f in (0.999, 1.001)]
        assert r[0] < MC.RATIO_GATE < r[1], (n, r)


def test_nonfinite_and_bad_match_cases(oracle, synth):
    c = MC.nonfinite(synth)
    assert len(c["where"]) == 5 * 4 * 5 and len(set(c["where"].tolist())) == 100 and len(c["nonfinite"]) == 60
    assert {int(i) // 64 for i in c["where"] if i < 256} == {0, 1, 2, 3} and (c["where"] >= 512).sum() == 20 and MC.NONFINITE_N % 256
    bad = np.stack(c["bad"]); good = np.stack(c["good"])
    assert np.isfinite(good).all() and (~np.isfinite(bad)).sum() == 60 and (np.abs(bad) == np.float32(3e38)).sum() == 40
    for k in range(4):                                   # every value in every coordinate
        col = bad[k, c["where"]]
        assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any() and (col == np.float32(3e38)).any() and (col == np.float32(-3e38)).any()
    with np.errstate(all="ignore"):
        xyz, ok = oracle.triangulate_stereo(*c["bad"], *c["K5"])
    assert not ok[c["nonfinite"]].any()
    keep = np.ones(len(ok), bool); keep[c["where"]] = False
    assert ok[keep].mean() > 0.95
    m = MC.bad_matches(synth)
    cap = m["cap"]
    assert MC.KP.itemsize == 28 and {cap + 1, MC.I32_MAX, -1, MC.I32_MIN, 2 * cap} <= set(m["nl"].tolist())
    for b in range(len(m["nl"])):
        assert {-1, cap, cap + 7, MC.I32_MAX, MC.I32_MIN} <= set(m["match"][b].tolist())
        bad_at = np.flatnonzero((m["match"][b] < 0) | (m["match"][b] >= cap))
        assert len(bad_at) == 5 and (np.diff(bad_at) > 1).all()          # valid indices beside them
    for k in ("kl", "kr"):
        for f in ("size", "angle", "response"):
            assert np.isnan(m[k][f]).any() and (m[k][f].view(np.uint32) != m[k + "_clean"][f].view(np.uint32)).mean() > 0.9
        assert (m[k]["octave"] != 0).mean() > 0.9 and (m[k]["class_id"] != 0).mean() > 0.9
        assert np.array_equal(m[k]["x"], m[k + "_clean"]["x"]) and np.array_equal(m[k]["y"], m[k + "_clean"]["y"])
    xyz, ok, written = MC.bad_matches_expected(oracle, m)
    assert written.sum() == sum(MC.clamp(n, cap) for n in m["nl"]) and ok[written].mean() > 0.8 and not ok[~written].any()


# ------------------------------------------------------------------------------------------------------------------------ fault rejection
def _numpy_matcher(q, t, fault=None):
    """the oracle's matcher restated on the kernel's quantities (dot = 256 - 2 d, packed best = dot * 32 + 31 - row % 32, chunks of 32 rows),
    with one optional fault"""
    nq, nt = len(q), len(t)
    if nt == 0:
        return np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    if fault == "tail_rows_as_zero":
        t = np.concatenate([t, np.zeros((-nt % 32, 32), np.uint8)])
    d = MC.popcount(q[:, None, :], t[None, :, :]).astype(np.int64)
    if fault == "last_index":
        idx = d.shape[1] - 1 - d[:, ::-1].argmin(1)
    elif fault == "later_chunk_wins":
        idx = np.zeros(nq, np.int64); best = np.full(nq, 1 << 30)
        for c0 in range(0, d.shape[1], 32):
            j = d[:, c0:c0 + 32].argmin(1) + c0
            v = d[np.arange(nq), j]
            take = v <= best                            # `>=` on the dot for `>`
            idx, best = np.where(take, j, idx), np.where(take, v, best)
    else:
        idx = d.argmin(1)
    dist = d[np.arange(nq), idx]
    if fault == "logical_shift":
        v = ((256 - 2 * dist) * 32 + 31 - idx % 32).astype(np.int32)
        dot = (v.view(np.uint32) >> 5).astype(np.int64)  # wrong for a negative packed best only
        dist = (256 - dot) >> 1
    if fault == "256_is_no_match":
        idx, dist = np.where(dist == 256, -1, idx), np.where(dist == 256, -1, dist)
    return idx.astype(np.int32), dist.astype(np.int32)


def _stand_in(case, fault):
    q, nq, t, nt, ei, ed = case
    cap = q.shape[1]
    gi = np.full_like(ei, MC.SENTINEL); gd = np.full_like(ed, MC.SENTINEL)
    for b in range(len(nq)):
        n, m = MC.clamp(nq[b], cap), MC.clamp(nt[b], cap)
        gi[b, :n], gd[b, :n] = _numpy_matcher(q[b, :n], t[b, :m], fault)
    return gi, gd


def test_rehearsal_a_faultless_matcher_stand_in_passes(oracle, cases):
    for name, case in cases.items():
        check_hamming(oracle, case, *_stand_in(case, None), name)
    for name in ("suffix_ties", "pair_ties"):            # a fault that needs a distance above 128 is invisible where there is none
        check_hamming(oracle, cases[name], *_stand_in(cases[name], "logical_shift"), name)


@pytest.mark.parametrize("fault,builders", [("last_index", ["suffix_ties", "pair_ties"]), ("later_chunk_wins", ["suffix_ties", "pair_ties"]),
                                            ("logical_shift", ["distance_ladder"]), ("tail_rows_as_zero", ["distance_ladder"]),
                                            ("256_is_no_match", ["distance_ladder"])])
def test_rehearsal_faulty_matchers_are_rejected(oracle, cases, fault, builders):
    for name in builders:
        with pytest.raises(AssertionError, match=name):
            check_hamming(oracle, cases[name], *_stand_in(cases[name], fault), name)


def test_rehearsal_every_tie_item_catches_a_wrong_tie_rule(oracle, cases):
    """not just one item of the builder: each listed pair rejects `last index`, each pair that spans two chunks rejects `later chunk wins`"""
    q, nq, t, nt, ei, ed = cases["pair_ties"]
    for b, (rows, n_t) in enumerate(MC.PAIR_TIES):
        one = tuple(a[b:b + 1] for a in (q, nq, t, nt, ei, ed))
        with pytest.raises(AssertionError):
            check_hamming(oracle, one, *_stand_in(one, "last_index"), "pair")
        if rows[0] // 32 != rows[-1] // 32:
            with pytest.raises(AssertionError):
                check_hamming(oracle, one, *_stand_in(one, "later_chunk_wins"), "pair")
    q, nq, t, nt, ei, ed = cases["distance_ladder"]
    for m in range(129, 257):                             # every distance above 128 rejects the logical shift
        one = tuple(a[m:m + 1] for a in (q, nq, t, nt, ei, ed))
        with pytest.raises(AssertionError):
            check_hamming(oracle, one, *_stand_in(one, "logical_shift"), "ladder")


def _tri_stand_in(L, fault):
    """the oracle's answer with the ratio or the vector taken from numpy's SVD of the same 4 x 4 matrix, wrongly"""
    ref = L["ref"]
    xyz, ok = ref["xyz"].copy(), ref["ok"].copy()
    if fault is None:
        return xyz, ok.astype(np.uint8)
    b = L["K5"][4]
    with np.errstate(all="ignore"):
        for i in range(len(ok)):
            u = MC.normalised(L["K5"], (L["xl"][i], L["yl"][i], L["xr"][i], L["yr"][i]))
            A = np.array([[-1, 0, u[0], 0], [0, -1, u[1], 0], [-1, 0, u[2], b], [0, -1, u[3], 0]], np.float64)
            _, s, Vt = np.linalg.svd(A)
            if fault == "ratio_over_largest":
                ok[i] = s[3] / s[0] < MC.RATIO_GATE and xyz[i, 2] > 0
            else:
                xyz[i] = Vt[2, :3] / Vt[2, 3]
    return xyz, ok.astype(np.uint8)


def test_rehearsal_faulty_triangulations_are_rejected(oracle, synth):
    L = MC.gate_ladder(oracle, synth, "kitti00")
    fig = check_tri(L["ref"], *_tri_stand_in(L, None), "faultless")
    assert fig["max_dev_over_bar"] == 0 and fig["compared"] >= 100
    with pytest.raises(AssertionError, match="decision differs"):
        check_tri(L["ref"], *_tri_stand_in(L, "ratio_over_largest"), "s_min / s_max")
    with pytest.raises(AssertionError, match="accepted with z <= 0|xyz beyond the bar"):
        check_tri(L["ref"], *_tri_stand_in(L, "second_smallest_vector"), "second-smallest column")
    xyz, ok = _tri_stand_in(L, "second_smallest_vector")
    keep = L["ref"]["stable"]                              # ... and on the stable cases alone it is the points that give it away
    with pytest.raises(AssertionError, match="xyz beyond the bar"):
        check_tri({k: v[keep] for k, v in L["ref"].items()}, xyz[keep], ok[keep], "second-smallest column, stable cases")
    xyz, ok = _tri_stand_in(L, None)                      # ... and the helper's other rules
    ok2 = ok.copy(); ok2[np.flatnonzero(~L["ref"]["stable"])[0]] = 2
    with pytest.raises(AssertionError, match="neither 0 nor 1"):
        check_tri(L["ref"], xyz, ok2, "ok = 2")
    i = np.flatnonzero(L["ref"]["stable"] & L["ref"]["ok"])[0]
    xyz[i, 2] *= 1 + 1e-7
    with pytest.raises(AssertionError, match="xyz beyond the bar"):
        check_tri(L["ref"], xyz, ok, "1e-7 off")
