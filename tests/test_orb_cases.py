"""CPU proof of tests/orb_cases.py on the oracle alone: every builder reaches the regime it is named for (asserted with the oracle's stage functions
grid_fast, fast_detect, fast_score_px, is_fast_corner, octree, ic_angle, sincos, brief, screen, detect, detect_and_compute), and two restatements
that are not the oracle's code agree with it: the FAST score from its definition (orb_cases.fast_score_definition) on every pixel of the arcs,
extremes and threshold_ladder images, and the patch moments in int64 with atan2 in float64 against ic_angle, within the measured deviation of
cv::fastAtan2 (orb_cases.ATAN2_BOUND_DEG) and exactly on the axes.  No GPU."""
import numpy as np
import pytest

import orb_cases as oc

B = oc.BORDER


def _cands(oracle, c):
    x, y, s = oracle.grid_fast(c.img, c.ini, c.mn)
    return list(zip(x.tolist(), y.tolist(), s.tolist()))


def _oracle_fallback(oracle, c):
    """cells whose candidates exist only at the minimum threshold, asked of the oracle's FAST cell by cell"""
    h, w = c.img.shape
    out = []
    for i, j, x0, x1, y0, y1 in oc.grid(h, w):
        roi = c.img[y0 - 3:y1 + 3, x0 - 3:x1 + 3]
        if len(oracle.fast_detect(roi, c.ini)[0]) == 0 and len(oracle.fast_detect(roi, c.mn)[0]) > 0:
            out.append((i, j))
    return out


def _assert_closed_form(oracle, c):
    got = _cands(oracle, c)
    assert got == c.known["cands"], (c.name, sorted(set(got) ^ set(c.known["cands"]))[:6])
    assert _oracle_fallback(oracle, c) == c.known["fallback"], c.name
    return got


# ------------------------------------------------------------------------------------------------------------------------ FAST
def test_threshold_ladder(oracle):
    cases = oc.threshold_ladder()
    assert [(c.ini, c.mn) for c in cases] == [(20, 7), (30, 10), (12, 5)]
    for c in cases:
        got = _assert_closed_form(oracle, c)
        ds = c.known["contrasts"]
        assert set(oc.LADDER) <= set(ds) and set(-d for d in oc.LADDER) <= set(ds) and len(ds) == len(oc.grid(oc.H, oc.W)) == 20
        # one dot per cell: a candidate of score |d| - 1 from mn on, through the fallback below ini
        assert sorted(s for _, _, s in got) == sorted(abs(d) - 1 for d in ds if abs(d) - 1 >= c.mn)
        assert len(c.known["fallback"]) == sum(1 for d in ds if c.mn <= abs(d) - 1 < c.ini) > 0
        scores = [s for _, _, s in got]
        assert c.ini - 1 in scores and c.ini in scores and c.mn in scores and c.mn - 1 not in scores
    first = {(x, y): s for x, y, s in _cands(oracle, cases[0])}
    assert sorted(first.values()).count(19) == 3 and sorted(first.values()).count(20) == 3        # d = +-20, +-21 and the two named against ini


def test_fallback_cells(oracle):
    c, = oc.fallback_cells()
    got = _assert_closed_form(oracle, c)
    assert c.known["fallback"] == c.known["weak_only"]
    cols = {j for i, j in c.known["weak_only"] if i == 0}
    assert cols == {0, 3, 4}                                            # first and last cell of the 4-cell strip, and the strip of one cell
    by_cell = {}
    for x, y, s in got:
        by_cell.setdefault(oc.cell_of(oc.H, oc.W, x + B, y + B), []).append(s)
    assert by_cell[(0, 1)] == [59] and by_cell[(0, 2)] == [20]          # the weak dot beside a strong one, and the 19 beside the 20, are dropped
    assert by_cell[(2, 0)] == [19] and by_cell[(2, 1)] == [20] and by_cell[(2, 3)] == [7] and (2, 2) not in by_cell
    assert sorted(by_cell[(1, 3)]) == [7, 12, 19] and len(by_cell[(1, 1)]) == 9
    assert all(cell not in by_cell for cell in ((1, 0), (1, 2), (2, 4), (2, 2)))
    assert set(by_cell) >= {(3, 0), (3, 2), (3, 4)}


def _compass(img, x, y, th):
    """the pre-test of the two-phase path (isFastCorner, ORBextractor.cpp:478-493): every opposite pair of ring pixels has one beyond v +- th"""
    v = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in oc.RING]
    return any(all(f(ring[k]) or f(ring[k + 8]) for k in range(8)) for f in (lambda p: p > v + th, lambda p: p < v - th))


def test_arcs(oracle):
    bright, dark, exact = oc.arcs()
    for c in (bright, dark):
        cand = {(x + B, y + B): s for x, y, s in _cands(oracle, c)}
        runs = {}
        for x, y, run, score in c.known["centres"]:
            assert oracle.fast_score_px(c.img, x, y) == score, (c.name, x, y, run)
            assert oracle.is_fast_corner(c.img, x, y, c.ini) == (run >= 9)
            assert ((x, y) in cand) == (run >= 9) and (run < 9 or cand[(x, y)] == oc.ARC_CONTRAST - 1)
            if run >= 8 and score in (-1, oc.ARC_CONTRAST - 1):
                assert _compass(c.img, x, y, c.ini), (x, y, run)        # passes the true corners AND the single runs of 8: the score rejects those
            runs[run] = runs.get(run, 0) + 1
        assert runs == {8: 17, 9: 16, 10: 16, 16: 1, 7: 1}
    cand = {(x + B, y + B): s for x, y, s in _cands(oracle, exact)}
    for x, y, run, score in exact.known["centres"]:
        assert oracle.fast_score_px(exact.img, x, y) == score
        assert not oracle.is_fast_corner(exact.img, x, y, score + 1) and oracle.is_fast_corner(exact.img, x, y, score)
        assert ((x, y) in cand) == (score >= exact.mn)
    assert sorted(s for _, _, _, s in exact.known["centres"]) == [6, 6, 7, 7, 19, 19, 20, 20]


def test_extremes(oracle):
    for c in oc.extremes():
        got = _assert_closed_form(oracle, c)
        scores = sorted(s for _, _, s in got)
        assert set(oc.EXTREME_SCORES) <= set(scores) and scores.count(254) == 1 + 8 + 2
        assert scores.count(7) == 2 and all(k in got for k in c.known["seam_sevens"])      # a 7 beside a 254 survives only across a seam
        assert c.known["fallback"] == [(3, 1), (3, 2)]
        assert {int(c.img.min()), int(c.img.max())} == {0, 255}
        pairs = [(x, y) for (x, y), s in c.known["scores"].items() if s == 7 and y < 115]
        assert {x % 4 for x, y in pairs} == {0, 1, 2, 3} and len(pairs) == 8


def _in_one_cell(h, w, pixels):
    cells = {oc.cell_of(h, w, x, y) for x, y in pixels}
    return len(cells) == 1 and None not in cells


def test_plateaus(oracle):
    c, = oc.plateaus()
    got = _assert_closed_form(oracle, c)
    cand = {(x + B, y + B): s for x, y, s in got}
    phases = {}
    for kind, x, y in c.known["placed"]:
        px = [(x + dx, y + dy) for dx, dy, _ in oc.PLATEAU_KINDS[kind]]
        assert _in_one_cell(oc.H, oc.W, px), (kind, x, y)               # seams are test_seams' matter
        phases.setdefault(kind, set()).add((x % 4, y % 2))
        alive = sorted(cand[p] for p in px if p in cand)
        want = {"block3": [59], "larger_diagonal": [54], "larger_antidiagonal": [54]}.get(kind, [])
        assert alive == want, (kind, x, y, alive)
    assert all(phases[k] == {(px, py) for px in range(4) for py in range(2)} for k in oc.PLATEAU_KINDS), phases


def test_seams(oracle):
    for c in oc.seams():
        h, w = c.img.shape
        got = _assert_closed_form(oracle, c)
        cand = {(x + B, y + B): s for x, y, s in got}
        st = c.known["straddle"]
        assert all(p in cand for p in st), [p for p in st if p not in cand]
        for a, b in zip(st[0::2], st[1::2]):                            # each pair: 8-neighbours in two different cells
            assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 and oc.cell_of(h, w, *a) != oc.cell_of(h, w, *b)
        ax, ay = c.known["inner"]
        assert (ax + 9, ay + 8) in cand and (ax + 8, ay + 8) not in cand            # inside a cell only the larger one
        assert (ax + 16, ay + 8) in cand and (ax + 16, ay + 9) not in cand
        assert (ax + 8, ay + 16) not in cand and (ax + 9, ay + 16) not in cand      # ... and neither of two equal ones
        assert cand[(19, 19)] == 56 and cand[(w - 20, h - 20)] == 57
        assert set(cand.values()) >= {44, 45, 46, 47, 49, 50, 51, 52, 53, 55, 56, 57}     # the dots on the first / last columns and rows
        lx0, lx1, ly0, ly1 = c.known["last_cell"]
        assert lx1 - lx0 < c.known["cell_width"]
    assert [c.known["cell_width"] % 2 for c in oc.seams()] == [0, 1]


# ------------------------------------------------------------------------------------------------------------------------ oct-tree
def _tree(oracle, c, cands=None):
    """the oracle's oct-tree on the closed-form candidates -> [(x, y, response)] in pixels"""
    cands = c.known["cands"] if cands is None else cands
    h, w = c.img.shape
    x, y, s = (np.array(v, np.int32) for v in zip(*cands))
    sel = oracle.octree(x, y, s, B, w - B, B, h - B, c.nfeatures)
    return [(int(x[i]) + B, int(y[i]) + B, int(s[i])) for i in sel]


def _detected(oracle, c):
    k = oracle.detect(c.params(oracle), c.img)
    return [(int(a), int(b), int(r)) for a, b, r in zip(k["x"], k["y"], k["response"])]


def _assert_tree(oracle, c):
    _assert_closed_form(oracle, c)
    assert c.known["fallback"] == [] and len(c.known["cands"]) == len(c.known["scores"])      # every dot is a candidate
    want = _tree(oracle, c)
    assert _detected(oracle, c) == want
    return want


def test_octree_split_lines(oracle):
    sizes = []
    for c in oc.octree_split_lines():
        got = _assert_tree(oracle, c)
        xs = {x for x, _, _ in c.known["cands"]}; ys = {y for _, y, _ in c.known["cands"]}
        assert {L + o for L in (42, 84, 126) for o in (-1, 0, 1)} <= xs and {L + o for L in (32, 64, 96) for o in (-1, 0, 1)} <= ys
        assert c.nfeatures <= len(got) < 72
        sizes.append(len(got))
    assert sizes == sorted(sizes) and len(set(sizes)) == 3
    # a dot ON a line belongs to the right / lower child (x < line goes left): the root's four children hold 15, 21, 15, 21 dots
    c = oc.octree_split_lines()[0]
    quad = [sum(1 for x, y, _ in c.known["cands"] if (x < 84) == left and (y < 64) == top) for top in (True, False) for left in (True, False)]
    assert sum(quad) == 72 and quad != [18, 18, 18, 18], quad


def test_octree_budgets(oracle):
    n = {}
    for c in oc.octree_budgets():
        n[(c.known["roots"], c.nfeatures)] = _assert_tree(oracle, c)
    # the first round splits every node whatever the budget; it ends the tree when the budget is met
    assert [len(n[(1, k)]) for k in (1, 2, 3, 4, 5)] == [4, 4, 4, 4, 7]
    assert [len(n[(11, k)]) for k in (10, 11, 12, 43, 44, 45)] == [44, 44, 44, 44, 44, 45]
    # 45: all 44 nodes hold two dots; the last-made one (bottom right of the last root) is split
    extra = set(n[(11, 45)]) - set(n[(11, 44)])
    hx = (1010 - 32) / 11
    assert len(extra) == 1 and all(x - B >= int(hx * 10) + 45 and y - B >= 43 for x, y, _ in extra), extra


def test_octree_equal_responses(oracle):
    for c in oc.octree_equal_responses():
        got = _assert_tree(oracle, c)
        assert {s for _, _, s in c.known["cands"]} == {39} and c.nfeatures <= len(got) < 130
        assert set(_tree(oracle, c, c.known["cands"][::-1])) != set(got)          # order-sensitive: every best-of-node is the first of its node


def test_octree_equal_sizes(oracle):
    c, = oc.octree_equal_sizes()
    got = {(x - B, y - B) for x, y, _ in _assert_tree(oracle, c)}
    assert len(got) == 6 and set(c.known["right"]) <= got and len(got & set(c.known["left"])) == 1


def test_octree_deep(oracle):
    shallow, mid, all_of_them = oc.octree_deep()
    for c in (shallow, mid, all_of_them):
        got = _assert_tree(oracle, c)
        dense = [(x, y) for x, y, _ in got if x - B < 40 and y - B < 36]
        assert len(got) - len(dense) == 6                                # the single dots all come back
        if c is all_of_them:
            assert len(got) == c.known["ndots"] < c.nfeatures            # nothing left to split: the tree ends below its budget
        else:
            assert c.nfeatures <= len(got) < c.known["ndots"]
    dense = sorted((x, y) for x, y, _ in _tree(oracle, mid) if x - B < 40 and y - B < 36)
    assert any(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 4 for a in dense for b in dense)          # lattice neighbours in separate nodes: 4-pixel nodes


def test_octree_wide(oracle):
    hx = np.float32(1010 - 32) / np.float32(11)
    few, many = oc.octree_wide()
    for c in (few, many):
        got = _assert_tree(oracle, c)
        xs = [x for x, _, _ in c.known["cands"]]
        per_root = [sum(1 for x in xs if int(np.float32(x) / hx) == r) for r in range(11)]
        assert per_root == [2, 4, 4, 2, 1, 2, 2, 0, 2, 4, 2], per_root   # a root without candidates among roots with one and with several
        for r in (1, 2, 3, 6, 9, 10):                                    # the borders that carry dots: the pixel ON int(hX * r) still divides into root r - 1
            b = int(hx * np.float32(r))
            assert {b - 1, b, b + 1, b + 2} <= set(xs)
            assert [int(np.float32(x) / hx) for x in (b - 1, b, b + 1)] == [r - 1, r - 1, r]
    # budget 9: the first round splits the 9 roots that hold more than one dot and ends the tree, one key-point per non-empty quadrant;
    # budget 30: more than the 25 dots, so the tree ends when nothing is left to split
    quadrants = set()
    for x, y, _ in few.known["cands"]:
        r = int(np.float32(x) / hx)
        ul, ur = int(hx * np.float32(r)), int(hx * np.float32(r + 1))
        quadrants.add((r, x < ul + -(-(ur - ul) // 2), y < 43))
    assert len(_tree(oracle, few)) == len(quadrants) - 0 == 13 and len(_tree(oracle, many)) == 25 == len(many.known["cands"])


# ------------------------------------------------------------------------------------------------------------------------ orientation
def _bits(a):
    return np.float32(a).view(np.uint32)


def test_axis_angles(oracle):
    seen, levels = set(), np.zeros(3, int)
    for c in oc.axis_angles():
        k, _ = oracle.detect_and_compute(c.params(oracle), c.img)
        levels += np.bincount(k["octave"], minlength=3)
        assert (np.bincount(k["octave"], minlength=3) > 0).all(), c.name             # the stamps are large enough for levels 1 and 2
        l0 = {(int(a["x"]), int(a["y"])): a["angle"] for a in k[k["octave"] == 0]}
        h, w = c.img.shape
        for x, y, d, side in c.known["stamps"]:
            assert min(x, y, w - 1 - x, h - 1 - y) == 19 and (x, y) in l0, (c.name, x, y)
            axis = (oc.AXIS_DEG[d] + (180 if c.known["dark"] else 0)) % 360
            m01, m10 = oc.moments(c.img, x, y)
            got = l0[(x, y)]
            assert _bits(got) == _bits(oracle.ic_angle(c.img, x, y))
            if side == 0:
                assert (m01 == 0) != (m10 == 0) and _bits(got) == _bits(axis) == _bits(oc.angle_deg64(m01, m10)), (c.name, x, y, got)
            else:
                assert min(abs(m01), abs(m10)) == 1 and got != np.float32(axis)
                assert abs((float(got) - axis + 180) % 360 - 180) < 0.002 and abs(float(got) - oc.angle_deg64(m01, m10)) <= oc.ATAN2_BOUND_DEG
            seen.add(float(got))
        for blob in filter(None, (c.known["blob"], (64, 80))):
            assert oc.moments(c.img, *blob) == (0, 0) and _bits(l0[blob]) == _bits(0.0) == _bits(oracle.fast_atan2(0.0, 0.0))
        if "extreme" in c.name:
            x, y, _, _ = c.known["stamps"][0]
            assert {0, 255} <= set(np.unique(c.img[y - 15:y + 16, x - 15:x + 16]).tolist())            # p - 128 = -128 and +127 in one patch
        # the second orientation implementation (ScreenAndComputeKPsParams) meets the same key-points
        s = oracle.screen(c.params(oracle), c.img, k)
        s0 = {(int(a["x"]), int(a["y"])): a["angle"] for a in s[s["octave"] == 0]}
        assert all(_bits(s0[p]) == _bits(l0[p]) for p in l0)
    assert {0.0, 90.0, 180.0, 270.0} <= seen
    for axis in (0.0, 90.0, 180.0, 270.0):                               # the nearest angles either side of every axis
        near = sorted((a - axis + 180) % 360 - 180 for a in seen if 0 < abs((a - axis + 180) % 360 - 180) < 0.01)
        assert near and near[0] < 0 < near[-1], (axis, near)
    assert 359.99 < max(seen) < 360.0
    assert (levels[1:] > 0).all()


def test_moments_restatement_against_ic_angle(oracle):
    """int64 moments + float64 atan2 against the oracle's IC_Angle on every level-0 key-point of the orientation and descriptor cases"""
    worst, n = 0.0, 0
    for c in oc.axis_angles() + oc.brief_ties():
        k, _ = oracle.detect_and_compute(c.params(oracle), c.img)
        for a in k[k["octave"] == 0]:
            x, y = int(a["x"]), int(a["y"])
            m01, m10 = oc.moments(c.img, x, y)
            assert _bits(a["angle"]) == _bits(oracle.fast_atan2(float(m01), float(m10))), (c.name, x, y, m01, m10)
            dev = abs((float(a["angle"]) - oc.angle_deg64(m01, m10) + 180) % 360 - 180)
            worst = max(worst, dev); n += 1
    assert n > 500 and worst <= oc.ATAN2_BOUND_DEG, (n, worst)


def _atan2_sweep(oracle, scale):
    r = np.arange(-260, 261)
    worst = (0.0, 0, 0)
    for m01 in r:
        got = np.array([oracle.fast_atan2(float(m01 * scale), float(m10 * scale)) for m10 in r], np.float64)
        ref = np.degrees(np.arctan2(float(m01 * scale), (r * scale).astype(np.float64))) % 360.0
        dev = np.abs((got - ref + 180) % 360 - 180)
        if m01 == 0:
            dev[260] = 0.0                                               # (0, 0): 0 by definition on both sides
        i = int(dev.argmax())
        if dev[i] > worst[0]:
            worst = (float(dev[i]), int(m01), int(r[i]))
    return worst


def test_fast_atan2_deviation_bound(oracle):
    """the measurement behind ATAN2_BOUND_DEG: integer moments of all octants at two magnitudes, and the exact values on the axes"""
    worst = max(_atan2_sweep(oracle, 1), _atan2_sweep(oracle, 64))
    print("largest deviation of fast_atan2 from float64 atan2 (degrees, m01, m10):", worst)
    assert np.ceil(worst[0] / 0.05) * 0.05 == oc.ATAN2_BOUND_DEG, worst
    for m in (1, 7, 36000, 91440, 1 << 24):
        got = [oracle.fast_atan2(0.0, float(m)), oracle.fast_atan2(float(m), 0.0), oracle.fast_atan2(0.0, float(-m)), oracle.fast_atan2(float(-m), 0.0)]
        assert [_bits(g) for g in got] == [_bits(a) for a in (0.0, 90.0, 180.0, 270.0)]
    assert 359.99 < oracle.fast_atan2(-1.0, 36013.0) < 360.0 and oracle.fast_atan2(-1.0, float(1 << 24)) <= 360.0


# ------------------------------------------------------------------------------------------------------------------------ FAST score by definition
@pytest.mark.parametrize("builder", [oc.arcs, oc.extremes, oc.threshold_ladder], ids=lambda b: b.__name__)
def test_fast_score_definition_against_oracle(oracle, builder):
    for c in builder():
        mine = oc.fast_score_definition(c.img)
        h, w = c.img.shape
        theirs = np.array([[oracle.fast_score_px(c.img, x, y) for x in range(3, w - 3)] for y in range(3, h - 3)], np.int32)
        assert np.array_equal(mine[3:h - 3, 3:w - 3], theirs), (c.name, np.argwhere(mine[3:h - 3, 3:w - 3] != theirs)[:4].tolist())
        assert theirs.max() >= c.mn
        for th in (c.ini, c.mn):                                         # and the thresholded map the cells are cut from
            m = oracle.fast_score_map(c.img, th)
            assert np.array_equal(m[3:h - 3, 3:w - 3], np.where(theirs >= th, theirs, 0))


# ------------------------------------------------------------------------------------------------------------------------ BRIEF half-way roundings
def test_brief_numpy_restatement(oracle):
    """orb_cases.brief_numpy / brief_coordinates against the oracle's brief at assorted angles, the tie angles among them"""
    img = oracle.blur7(oc.tie_background(5), 0)
    pat = oracle.pattern()
    for i, ang in enumerate([0.0, 90.0, 180.0, 270.0, 359.99841, 33.3, 271.25] + [oc.tie_angle(k) for k in oc.TIE_ANGLES]):
        a, b = oc.rotation(oracle, ang)
        r, c = oc.brief_coordinates(pat, a, b)
        x, y = 40 + (i * 17) % 120, 40 + (i * 29) % 80
        mine = oc.brief_numpy(img, x, y, np.rint(r).astype(int), np.rint(c).astype(int))
        assert np.array_equal(mine, oracle.brief(img, x, y, float(ang))), ang


def test_brief_ties(oracle):
    cases = oc.brief_ties()
    assert 0 < len(cases) <= 16
    total = [oc.count_image_ties(oracle, c) for c in cases]
    assert all(t >= f >= 1 for t, f, _ in total), total
    assert sum(f for _, f, _ in total) >= 8, total                       # half-way coordinates whose other rounding changes a descriptor bit
    # each of the four roundings of a test is its own instruction in both implementations: every one meets coordinates that tell half-to-even
    # from half-away-from-zero (two each) and from truncation (any flipping coordinate)
    detail = [d for _, _, det in total for d in det]
    assert all(detail.count((slot, True)) >= 2 and detail.count((slot, False)) >= 1 for slot in oc.TIE_SLOTS), detail


def test_tie_angles(oracle):
    pat = oracle.pattern()
    assert len(oc.TIE_ANGLES) == 32 == len(set(oc.TIE_ANGLES))
    n = []
    for k in oc.TIE_ANGLES:
        r, c = oc.brief_coordinates(pat, *oc.rotation(oracle, oc.tie_angle(k)))
        n.append(int(oc.halfway(r).sum() + oc.halfway(c).sum()))
    assert min(n) >= 1 and sum(n) >= 64, n
    assert any(k % 16 == 0 for k in oc.TIE_ANGLES)                        # multiples of 360 / 65536 among them
    from pyoracle import KP_DTYPE
    img, kps = oc.tie_angle_keypoints(KP_DTYPE)
    p = oracle.params(oc.TIE_NFEATURES, 1.2, 3)
    pyr = oracle.pyramid(p, img)
    sc = oracle.orb_tables(p)[0]
    desc = oracle.calc_descriptors(p, img, kps)
    flips, detail = 0, []
    for k, d in zip(kps, desc):
        l = int(k["octave"])
        x, y = int(np.rint(k["x"] / sc[l])), int(np.rint(k["y"] / sc[l]))
        t, f, mine, det = oc.tie_report(oracle, pat, oracle.blur7(pyr[l], 0), x, y, k["angle"])
        assert t >= 1 and np.array_equal(mine, d)
        flips += f; detail += det
    assert flips >= 32, flips                                            # one per angle on average
    assert all(detail.count((slot, True)) >= 2 and detail.count((slot, False)) >= 1 for slot in oc.TIE_SLOTS), detail


def test_every_builder_is_asserted():
    """a regime assertion exists for every builder of orb_cases.ALL_BUILDERS"""
    names = {b.__name__ for b in oc.ALL_BUILDERS}
    assert names == {n[5:] for n in globals() if n.startswith("test_") and n[5:] in names}
    all_names = [c.name for c in oc.all_cases()]
    assert len(all_names) == len(set(all_names))
