"""Hand-made inputs of the ORB extractor (csrc/orb_kernels.hip: k_fast_strip, k_octree, describe_block, k_screen / k_pkf_screen, wave_brief) at small
sizes, for the decisions that textures, noise and rendered scenes reach only by chance: FAST scores at the fallback thresholds and at the top of a
byte, ring runs of exactly 8 and 9 pixels, equal scores side by side and across cell seams, oct-tree splits with candidates on the split lines and
budgets at the root counts, key-point angles exactly on the axes, and rotated BRIEF coordinates exactly half-way between two pixels.  No GPU here.
tests/test_orb_cases.py proves on the oracle alone that every case reaches the regime it is named for; tests/test_gpu_orb_edges.py runs the device
on the same inputs.

Images are 160 x 200 unless a case needs more.  At that size level 0 has 4 x 5 FAST cells of 32 x 34 pixels (the last row 26 high, the last column
26 wide: `grid`), the strip kernel takes the cells of a row four at a time (cells 0-3, then cell 4 alone), and the oct-tree has one root of
168 x 128 whose split lines are x = 84, y = 64 and then x = 42, 126, y = 32, 96 in the border-relative coordinates of the candidates (pixel - 16).

A flat image with ONE pixel changed by d gives exactly one candidate (x - 16, y - 16, |d| - 1): the ring of the pixel is flat, so all 16 differences
are d, and no other pixel has 9 contiguous ring pixels that differ from it.  Dots whose Chebyshev distance is 4 or more do not lie on each
other's rings, so an image of such dots has the closed-form candidate list `grid_candidates` computes from the dots alone.

Every builder returns a list of Case: the image, the extractor parameters, the regime's name and what the builder knows in closed form.

cv::fastAtan2 against float64 atan2: the largest deviation of the oracle's fast_atan2 over the integer moments (m01, m10) in [-260, 260]^2 and
64 x that (all octants, 271 441 pairs each) measured 0.009552 degrees, on the diagonals (m01 = m10 = -260: 225.00955)
(tests/test_orb_cases.py::test_fast_atan2_deviation_bound re-measures it); ATAN2_BOUND_DEG is that, rounded up to the next 0.05 degrees.  On the
axes and at (0, 0) the result is exact: 0, 90, 180, 270.

Run as a script (python tests/orb_cases.py) this module repeats the bounded searches whose results are committed below as TIE_STAMPS and
TIE_ANGLES; the tests never run them."""
import numpy as np

H, W = 160, 200
BG = 100
BORDER = 16                                            # EDGE_THRESHOLD - 3: candidates are relative to this pixel
ATAN2_BOUND_DEG = 0.05
# ring position k -> (dx, dy), ORBextractor.cpp:365-369
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]                  # half-widths of the rows of the 31-pixel patch


class Case:
    def __init__(self, name, regime, img, nfeatures, nlevels, ini=20, mn=7, scale=1.2, **known):
        self.name, self.regime, self.img = name, regime, np.ascontiguousarray(img, np.uint8)
        self.nfeatures, self.nlevels, self.ini, self.mn, self.scale = nfeatures, nlevels, ini, mn, scale
        self.known = known                             # closed-form facts: cands, fallback, centres, ...

    @property
    def config(self):
        return (self.nfeatures, self.scale, self.nlevels, self.ini, self.mn)

    def params(self, oracle):
        return oracle.params(self.nfeatures, self.scale, self.nlevels, self.ini, self.mn)

    def extractor(self, api):
        return api.ORBextractor(self.nfeatures, self.scale, self.nlevels, self.ini, self.mn)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------------------------------ geometry
def grid(h, w):
    """FAST cells of a level, ORBextractor.cpp:814-843, as (row, col, x0, x1, y0, y1): the cell reports pixels [x0, x1) x [y0, y1), and its
    non-maximum suppression sees no score outside them"""
    bw, bh = w - 2 * BORDER, h - 2 * BORDER
    nc, nr = bw // 30, bh // 30
    wc, hc = -(-bw // nc), -(-bh // nr)
    cells = []
    for i in range(nr):
        y0 = BORDER + i * hc
        if y0 >= h - BORDER - 3:
            continue
        y1 = min(y0 + hc + 6, h - BORDER)
        for j in range(nc):
            x0 = BORDER + j * wc
            if x0 >= w - BORDER - 6:
                continue
            x1 = min(x0 + wc + 6, w - BORDER)
            cells.append((i, j, x0 + 3, x1 - 3, y0 + 3, y1 - 3))
    return cells


def cell_of(h, w, x, y):
    for i, j, x0, x1, y0, y1 in grid(h, w):
        if x0 <= x < x1 and y0 <= y < y1:
            return i, j
    return None


def grid_candidates(scores, h, w, ini, mn):
    """Closed form of the grid FAST from the scores of the changed pixels alone ({(x, y): score}; every other pixel scores below mn):
    per cell strict 3 x 3 non-maximum suppression among the scores >= ini, and among those >= mn when that leaves nothing.
    -> (candidates (x - 16, y - 16, score) in cell order, cells whose candidates come from the fallback)"""
    out, fallback = [], []
    for i, j, x0, x1, y0, y1 in grid(h, w):
        inside = {p: s for p, s in scores.items() if x0 <= p[0] < x1 and y0 <= p[1] < y1}
        for th in (ini, mn):
            live = {p: s for p, s in inside.items() if s >= th}
            keep = [p for p, s in live.items()
                    if all(s > live.get((p[0] + dx, p[1] + dy), 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy)]
            if keep:
                break
        if keep and th != ini:
            fallback.append((i, j))
        out += [(x - BORDER, y - BORDER, live[(x, y)]) for x, y in sorted(keep, key=lambda p: (p[1], p[0]))]
    return out, fallback


class Dots:
    """a flat image and the pixels changed on it: put(x, y, d) sets the pixel to bg + d and records the score |d| - 1"""

    def __init__(self, h=H, w=W, bg=BG):
        self.img = np.full((h, w), bg, np.uint8)
        self.bg, self.scores = bg, {}

    def put(self, x, y, d, score=None):
        v = self.bg + d
        assert 0 <= v <= 255 and d != 0 and (x, y) not in self.scores, (x, y, d)
        self.img[y, x] = v
        self.scores[(x, y)] = abs(d) - 1 if score is None else score

    def rel(self, xr, yr, d):
        self.put(xr + BORDER, yr + BORDER, d)

    def case(self, name, regime, nfeatures, nlevels=1, ini=20, mn=7, **known):
        h, w = self.img.shape
        cands, fallback = grid_candidates(self.scores, h, w, ini, mn)
        return Case(name, regime, self.img, nfeatures, nlevels, ini, mn, cands=cands, fallback=fallback, scores=dict(self.scores), **known)


# ------------------------------------------------------------------------------------------------------------------------ FAST
LADDER = (6, 7, 8, 9, 19, 20, 21, 22)
LADDER_THRESHOLDS = ((20, 7), (30, 10), (12, 5))


def threshold_ladder():
    """one dot per cell: contrasts 6 .. 22 in both polarities (16 cells) and, in the four cells left, the contrasts that score exactly
    ini - 1, ini (bright) and mn - 1, mn (dark) of the case's own thresholds"""
    cells = grid(H, W)
    out = []
    for ini, mn in LADDER_THRESHOLDS:
        ds = [s * d for s in (1, -1) for d in LADDER] + [ini, ini + 1, -mn, -(mn + 1)]
        D = Dots()
        for k, (d, (i, j, x0, x1, y0, y1)) in enumerate(zip(ds, cells)):
            D.put(x0 + 5 + (k * 7) % (x1 - x0 - 10), y0 + 4 + (k * 5) % (y1 - y0 - 8), d)
        out.append(D.case(f"threshold_ladder[{ini},{mn}]", "ladder", 64, 1, ini, mn, contrasts=ds))
    return out


def fallback_cells():
    """what a cell can hold, by cell (row, col) of the 4 x 5 grid; scores are named against ini = 20 / mn = 7.  Row 0: weak only in cell 0 (the first
    of a 4-cell strip), weak + strong, 19 next to 20, weak only in cell 3 (the last of the strip) and in cell 4 (a strip of one cell).  Row 1: nothing,
    a full cell, nothing, three weak dots, strong.  Row 2: 19 alone, 20 alone, 6 alone (below mn: nothing), 7 alone, nothing.  Row 3 (26 pixels high):
    weak only in the first and the last cell, strong in the middle one."""
    D = Dots()
    c = {(i, j): (x0, y0) for i, j, x0, x1, y0, y1 in grid(H, W)}

    def at(cell, dx, dy, d):
        D.put(c[cell][0] + dx, c[cell][1] + dy, d)
    at((0, 0), 9, 9, 12); at((0, 0), 20, 17, -15)
    at((0, 1), 6, 6, 11); at((0, 1), 18, 14, 60)
    at((0, 2), 10, 10, 20); at((0, 2), 15, 10, 21)
    at((0, 3), 3, 25, -9); at((0, 3), 30, 2, 14)
    at((0, 4), 12, 12, 10); at((0, 4), 20, 20, 19)
    for k in range(9):
        at((1, 1), 4 + 10 * (k % 3), 5 + 9 * (k // 3), (25 + 8 * k) * (1 if k % 2 else -1))
    at((1, 3), 5, 5, 8); at((1, 3), 16, 12, -13); at((1, 3), 27, 24, 20)
    at((1, 4), 10, 15, 90)
    at((2, 0), 17, 16, 20)
    at((2, 1), 17, 16, 21)
    at((2, 2), 17, 16, 7)
    at((2, 3), 17, 16, -8)
    at((3, 0), 8, 8, 16); at((3, 4), 20, 20, -18); at((3, 2), 11, 11, 77)
    return [D.case("fallback_cells", "fallback", 64, weak_only=[(0, 0), (0, 3), (0, 4), (1, 3), (2, 0), (2, 3), (3, 0), (3, 4)])]


def _arc(img, cx, cy, start, length, delta):
    for k in range(start, start + length):
        dx, dy = RING[k % 16]
        img[cy + dy, cx + dx] = int(img[cy + dy, cx + dx]) + delta


ARC_PITCH, ARC_CONTRAST = 13, 30


def _arc_slots():
    return [(25 + ARC_PITCH * i, 25 + ARC_PITCH * j) for j in range(9) for i in range(12)]


def arcs():
    """centres (value 100) whose ring holds one contiguous run of 8, 9, 10 pixels 30 beyond them, starting at each of the 16 ring positions, the
    whole ring, a bright and a dark run of 8 side by side, and two runs of 7 with one-pixel gaps; one image per polarity.  known['centres'] =
    [(x, y, run, score)]: 29 with a run of 9 or more, -1 below (-31 between a bright and a dark run).  A third image holds runs of 9 at exactly v +- ini and v +- mn (scores ini - 1
    and mn - 1: no corner at that threshold) next to runs one grey level stronger, one per cell."""
    out = []
    for pol in (1, -1):
        img = np.full((H, W), BG, np.uint8)
        slots = iter(_arc_slots())
        centres = []
        for length in (8, 9, 10):
            for start in range(16):
                x, y = next(slots)
                _arc(img, x, y, start, length, pol * ARC_CONTRAST)
                centres.append((x, y, length, ARC_CONTRAST - 1 if length >= 9 else -1))
        x, y = next(slots); _arc(img, x, y, 0, 16, pol * ARC_CONTRAST); centres.append((x, y, 16, ARC_CONTRAST - 1))
        x, y = next(slots); _arc(img, x, y, 3, 8, pol * ARC_CONTRAST); _arc(img, x, y, 11, 8, -pol * ARC_CONTRAST); centres.append((x, y, 8, -1 - ARC_CONTRAST))
        x, y = next(slots); _arc(img, x, y, 5, 7, pol * ARC_CONTRAST); _arc(img, x, y, 13, 7, pol * ARC_CONTRAST); centres.append((x, y, 7, -1))
        out.append(Case("arcs[%s]" % ("bright" if pol > 0 else "dark"), "arcs", img, 200, 1, centres=centres))
    img = np.full((H, W), BG, np.uint8)
    centres = []
    cells = grid(H, W)
    for k, c in enumerate((20, 21, 7, 8, -20, -21, -7, -8)):
        i, j, x0, x1, y0, y1 = cells[2 * k]
        x, y = x0 + 10 + k, y0 + 12
        _arc(img, x, y, 2 * k, 9, c)
        centres.append((x, y, 9, abs(c) - 1))
    out.append(Case("arcs[exact]", "arcs", img, 200, 1, centres=centres))
    return out


def _slots(x0=21, y0=21, x1=W - 19, y1=H - 19, pitch=10, extent=6):
    return [(x, y) for y in range(y0, y1 - extent, pitch) for x in range(x0, x1 - extent, pitch)]


EXTREME_SCORES = (200, 211, 222, 233, 244, 250, 251, 252, 253, 254)


def extremes():
    """bg 0 with bright pixels and bg 255 with dark ones: single dots scoring 200 .. 254, horizontally adjacent pairs scoring (254, 7) and (7, 254)
    at the four x phases (one cell: only the 254 is a candidate), and the same pairs across the seams x = 52 | 53 and x = 120 | 121 of the last
    cell row, where the 7 sits alone in its cell and comes back through the fallback"""
    out = []
    for bg, sg in ((0, 1), (255, -1)):
        D = Dots(bg=bg)
        slots = iter(_slots(y1=115))
        for s in EXTREME_SCORES:
            x, y = next(slots)
            D.put(x, y, sg * (s + 1))
        for phase in range(4):
            for order in (0, 1):
                x, y = next(slots)
                D.put(x + phase, y + order, sg * (255 if order == 0 else 8))
                D.put(x + phase + 1, y + order, sg * (8 if order == 0 else 255))
        D.put(52, 125, sg * 255); D.put(53, 125, sg * 8)
        D.put(120, 126, sg * 8); D.put(121, 126, sg * 255)
        out.append(D.case(f"extremes[bg{bg}]", "extremes", 200, seam_sevens=[(53 - BORDER, 125 - BORDER, 7), (120 - BORDER, 126 - BORDER, 7)]))
    return out


# structures of equal and unequal neighbours: (dx, dy, contrast); `survivors` of one inside a cell follow from strict suppression
PLATEAU_KINDS = {
    "horizontal": [(0, 0, 40), (1, 0, 40)],
    "vertical": [(0, 0, 40), (0, 1, 40)],
    "diagonal": [(0, 0, 40), (1, 1, 40)],
    "antidiagonal": [(1, 0, 40), (0, 1, 40)],
    "block2": [(0, 0, 40), (1, 0, 40), (0, 1, 40), (1, 1, 40)],
    "block3": [(dx, dy, 60 if (dx, dy) == (1, 1) else 40) for dy in range(3) for dx in range(3)],
    "larger_diagonal": [(0, 0, 40), (1, 1, 55)],
    "larger_antidiagonal": [(1, 0, 55), (0, 1, 40)],
}


def plateaus():
    """every kind of PLATEAU_KINDS at the four x mod 4 and the two y mod 2 phases, each inside one cell (seams: `seams`), polarity alternating:
    equal neighbours suppress each other"""
    D = Dots()
    slots = iter((x, y) for x, y in _slots()                        # slots whose 6 x 4 pixels (structure + phase) lie inside ONE cell
                 if cell_of(H, W, x, y) is not None and cell_of(H, W, x, y) == cell_of(H, W, x + 5, y + 3))
    placed = []
    n = 0
    for kind, px in PLATEAU_KINDS.items():
        for phase in range(8):
            x, y = next(slots)
            sg = 1 if n % 2 == 0 else -1
            n += 1
            ox, oy = (phase % 4 - x) % 4, (phase // 4 - y) % 2          # the structure's origin at x mod 4 = phase % 4, y mod 2 = phase // 4
            for dx, dy, d in px:
                D.put(x + ox + dx, y + oy + dy, sg * d)
            placed.append((kind, x + ox, y + oy))
    return [D.case("plateaus", "plateaus", 300, placed=placed)]


def seams():
    """neighbour pairs (equal and unequal scores; horizontal, vertical, diagonal) straddling a cell border, where both survive, and the same pairs
    inside a cell; dots in the first and last column and row of a cell, of the last cell column and row (narrower than the others), and at the
    first and the last pixel of the level; a second image of 157 x 197 has cells 33 wide (odd) and the same furniture"""
    out = []
    for h, w in ((H, W), (157, 197)):
        D = Dots(h, w)
        cells = {(i, j): c for i, j, *c in grid(h, w)}
        x0, x1, y0, y1 = cells[(1, 1)]                              # an inner cell: its borders are seams on all four sides
        straddle = []
        for k, (da, db) in enumerate(((40, 40), (40, 55), (55, 40))):
            ya = y0 + 6 + 7 * k                                      # horizontal pairs across the left seam of cell (1, 1)
            D.put(x0 - 1, ya, da); D.put(x0, ya, db); straddle += [(x0 - 1, ya), (x0, ya)]
            xa = x0 + 6 + 7 * k                                      # vertical pairs across its top seam
            D.put(xa, y0 - 1, -da); D.put(xa, y0, -db); straddle += [(xa, y0 - 1), (xa, y0)]
        D.put(x1 - 1, y1 - 1, 40); D.put(x1, y1, 40); straddle += [(x1 - 1, y1 - 1), (x1, y1)]         # diagonal across the corner
        D.put(x1, y0 + 8, 33); D.put(x1 - 1, y0 + 9, 33); straddle += [(x1, y0 + 8), (x1 - 1, y0 + 9)]   # antidiagonal across the right seam
        ax0, ax1, ay0, ay1 = cells[(2, 2)]                           # the same pairs inside a cell
        D.put(ax0 + 8, ay0 + 8, 40); D.put(ax0 + 9, ay0 + 8, 55)
        D.put(ax0 + 16, ay0 + 8, -55); D.put(ax0 + 16, ay0 + 9, -40)
        D.put(ax0 + 8, ay0 + 16, 40); D.put(ax0 + 9, ay0 + 16, 40)
        bx0, bx1, by0, by1 = cells[(2, 0)]                           # first / last interior column and row of a cell
        D.put(bx0, by0 + 10, 45); D.put(bx1 - 1, by0 + 15, 46); D.put(bx0 + 10, by0, 47); D.put(bx0 + 15, by1 - 1, 48)
        lx0, lx1, ly0, ly1 = cells[(3, 4)]                           # the last cell of the level: narrower and lower than the others
        D.put(lx0, ly0 + 5, 50); D.put(lx0 + 12, ly0, 51); D.put(lx1 - 1, ly0 + 9, 52); D.put(lx0 + 7, ly1 - 1, 53)
        tx0, tx1, ty0, ty1 = cells[(0, 4)]
        D.put(tx1 - 1, ty0 + 11, 54)                                 # last column of the level, first cell row
        mx0, mx1, my0, my1 = cells[(3, 1)]
        D.put(mx0 + 13, my1 - 1, 56)                                 # last row of the level, an inner cell column
        D.put(19, 19, 57); D.put(w - 20, h - 20, 58)                 # first and last pixel of the level
        assert (lx1, ly1) == (w - 19, h - 19)
        out.append(D.case(f"seams[{h}x{w}]", "seams", 200, straddle=straddle, inner=(ax0, ay0), cell_width=x1 - x0, last_cell=(lx0, lx1, ly0, ly1)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ oct-tree
def _contrast(k):
    """distinct-looking strong contrasts, alternating polarity"""
    return (25 + (k * 37) % 71) * (1 if k % 2 == 0 else -1)


def _split_line_dots():
    D = Dots()
    k = 0
    for L in (42, 84, 126):
        for yb in (16, 48, 80, 112):
            for o in (-1, 0, 1):
                D.rel(L + o, yb + 5 * o, _contrast(k)); k += 1
    for L in (32, 64, 96):
        for xb in (21, 63, 105, 147):
            for o in (-1, 0, 1):
                D.rel(xb + 5 * o, L + o, _contrast(k)); k += 1
    return D


def octree_split_lines():
    """72 dots on the split lines x = 84, y = 64 of the root and x = 42, 126, y = 32, 96 of its children, and one pixel either side of them, with
    budgets that stop the tree after the first, second and third round"""
    D = _split_line_dots()
    return [D.case(f"octree_split_lines[{n}]", "octree", n) for n in (8, 20, 40)]


def octree_budgets():
    """budgets at the root count and at 4 x the root count, one below and above each: the one root of 160 x 200 (split_lines dots), and the 11
    roots of 118 x 1010 with two dots in every quadrant of every root — 44 nodes of two after the first round, so nfeatures = 45 splits exactly
    one of 44 nodes of equal size"""
    D = _split_line_dots()
    out = [D.case(f"octree_budgets[1root,{n}]", "octree", n, roots=1) for n in (1, 2, 3, 4, 5)]
    Dw = Dots(118, 1010)
    hx = np.float32(1010 - 32) / np.float32(11)
    k = 0
    for r in range(11):
        ul = int(hx * np.float32(r))
        for qx in (10, 54):
            for qy in (10, 55):
                Dw.rel(ul + qx, qy, _contrast(k)); Dw.rel(ul + qx + 10, qy + 15, _contrast(k + 1)); k += 2
    out += [Dw.case(f"octree_budgets[11roots,{n}]", "octree", n, roots=11) for n in (10, 11, 12, 43, 44, 45)]
    return out


def octree_equal_responses():
    """130 dots of one contrast on a 12-pixel lattice: every best-of-node is a tie, broken by the order of the candidates"""
    D = Dots()
    for yr in range(6, 121, 12):
        for xr in range(6, 161, 12):
            D.rel(xr, yr, 40)
    return [D.case(f"octree_equal_responses[{n}]", "octree", n) for n in (7, 30)]


def octree_equal_sizes():
    """children of 3, 3, 1, 1 candidates and a budget of 5: the two nodes of three compete for the last split; the later-made one (top right) is split"""
    D = Dots()
    for k, (xr, yr) in enumerate(((10, 10), (60, 12), (14, 50), (100, 8), (150, 14), (96, 52), (30, 100), (130, 96))):
        D.rel(xr, yr, _contrast(k))
    return [D.case("octree_equal_sizes", "octree", 5, left=[(10, 10), (60, 12), (14, 50)], right=[(100, 8), (150, 14), (96, 52)])]


def octree_deep():
    """72 dots on a 4-pixel lattice in one corner and single dots elsewhere: the dense node is split down to single pixels while the others stop;
    with a budget above the number of dots the tree ends because nothing is left to split"""
    D = Dots()
    k = 0
    for yr in range(4, 36, 4):
        for xr in range(4, 40, 4):
            D.rel(xr, yr, _contrast(k)); k += 1
    for xr, yr in ((120, 20), (20, 100), (110, 90), (150, 120), (70, 10), (10, 58)):
        D.rel(xr, yr, _contrast(k)); k += 1
    return [D.case(f"octree_deep[{n}]", "octree", n, ndots=k) for n in (20, 50, k + 5)]


def octree_wide():
    """118 x 1010, 11 roots: dots either side of the root borders (x / hX in float decides the root, int(hX * i) its corners); root 4 holds
    one dot, roots 5 and 8 the two left of their right border (the pixel ON int(hX * i) still divides into the root before), root 7 none"""
    D = Dots(118, 1010)
    hx = np.float32(1010 - 32) / np.float32(11)
    k = 0
    for r in range(1, 11):
        if r in (4, 5, 7, 8):
            continue
        b = int(hx * np.float32(r))
        for o, yr in ((-1, 10), (0, 30), (1, 50), (2, 70)):
            D.rel(b + o, yr, _contrast(k)); k += 1
    D.rel(int(hx * np.float32(4)) + 40, 40, _contrast(k))            # root 4: this dot alone
    return [D.case(f"octree_wide[{n}]", "octree", n, roots=11) for n in (9, 30)]


# ------------------------------------------------------------------------------------------------------------------------ orientation
DIRS = {"right": (1, 0), "down": (0, 1), "left": (-1, 0), "up": (0, -1)}            # where the bar lies, seen from the key-point
AXIS_DEG = {"right": 0.0, "down": 90.0, "left": 180.0, "up": 270.0}                 # angle of a bright bar; a dark one points the other way
BAR_LEN = 24


def stamp(img, x, y, direction, bar, centre, length=BAR_LEN, sat=None):
    """a bar 3 pixels wide and `length` long whose end pixel (x, y) has the value `centre`; sat = (along, side, delta) adds delta to the bar pixel
    `along` pixels from (x, y) on the row side = +-1 beside the axis"""
    ux, uy = DIRS[direction]
    vx, vy = -uy, ux                                                  # the side axis: u rotated by +90 degrees (x right, y down)
    for a in range(length + 1):
        for s in (-1, 0, 1):
            img[y + a * uy + s * vy, x + a * ux + s * vx] = bar
    img[y, x] = centre
    if sat:
        a, s, delta = sat
        yy, xx = y + a * uy + s * vy, x + a * ux + s * vx
        img[yy, xx] = int(img[yy, xx]) + delta


def blob(img, x, y, ring, centre, outer=None):
    """3 x 3 with a brighter centre, point-symmetric; with `outer` a 7 x 7 frame around it, which the upper levels still resolve"""
    if outer is not None:
        img[y - 3:y + 4, x - 3:x + 4] = outer
    img[y - 1:y + 2, x - 1:x + 2] = ring
    img[y, x] = centre


def _axis_layouts(h=H, w=W):
    """key-points exactly 19 pixels from a border: the four corners, and the middle of the four edges with a blob in the image centre"""
    corners = [(19, 19, "right"), (w - 20, 19, "down"), (w - 20, h - 20, "left"), (19, h - 20, "up")]
    edges = [(w // 2, 19, "down"), (w - 20, h // 2, "left"), (w // 2, h - 20, "up"), (19, h // 2, "right")]
    return {"corners": corners, "edges": edges}


def axis_angles():
    """bar stamps in the four directions with their key-points in the corners and at the edges of the level (19 pixels from the borders), plain
    (angles exactly 0, 90, 180, 270) and with one bar pixel one grey level up on either side of the axis, 13 pixels out (the angles next to the
    axes: |m01| = 1 against |m10| of the whole bar); a point-symmetric blob (both moments zero: angle 0); one set drawn with 0 / 254 / 255 and
    its negative, so the matrix-core operands p - 128 are -128 and +127.  known['stamps'] = [(x, y, direction, side)]"""
    out = []
    for lname, layout in _axis_layouts().items():
        for side in (0, 1, -1):
            img = np.full((H, W), BG, np.uint8)
            for x, y, d in layout:
                stamp(img, x, y, d, 200, 230, sat=(13, side, 1) if side else None)
            if lname == "edges":
                blob(img, W // 2, H // 2, 160, 220)
            blob(img, 64, 80, 190, 240, outer=150)
            out.append(Case(f"axis_angles[{lname},{'plain' if not side else 'sat%+d' % side}]", "axis", img, 100, 3,
                            stamps=[(x, y, d, side) for x, y, d in layout], blob=(W // 2, H // 2) if lname == "edges" else None, dark=False))
    for bg, bar, centre, dark in ((0, 254, 255, False), (255, 1, 0, True)):
        img = np.full((H, W), bg, np.uint8)
        layout = _axis_layouts()["edges"]
        for x, y, d in layout:
            stamp(img, x, y, d, bar, centre)
        blob(img, W // 2, H // 2, bar, centre)
        blob(img, 64, 80, bar, centre, outer=128)
        out.append(Case(f"axis_angles[extreme,bg{bg}]", "axis", img, 100, 3, stamps=[(x, y, d, 0) for x, y, d in layout], blob=(W // 2, H // 2), dark=dark))
    return out


def moments(img, x, y):
    """(m01, m10) of the 31-pixel circular patch in int64: sum of v * I and of u * I over |u| <= UMAX[|v|]"""
    m01 = m10 = 0
    for v in range(-15, 16):
        u = np.arange(-UMAX[abs(v)], UMAX[abs(v)] + 1, dtype=np.int64)
        row = img[y + v, x + u].astype(np.int64)
        m01 += v * int(row.sum())
        m10 += int((u * row).sum())
    return m01, m10


def angle_deg64(m01, m10):
    """float64 atan2 in degrees, [0, 360)"""
    a = np.degrees(np.arctan2(float(m01), float(m10)))
    return a + 360.0 if a < 0 else a


# ------------------------------------------------------------------------------------------------------------------------ FAST score by definition
def fast_score_definition(img):
    """score of every pixel at least 3 from the border (-1000 elsewhere), from the definition alone: the largest t for which 9 contiguous ring
    pixels are all > v + t or all < v - t.  The predicate is monotonic in t, so the largest t is found per pixel by bisection over [-256, 255]."""
    I = img.astype(np.int32)
    h, w = I.shape
    v = I[3:h - 3, 3:w - 3]
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])

    def corner_at(t):
        ok = np.zeros(v.shape, bool)
        for beyond in (ring > v + t, ring < v - t):
            run = np.concatenate([beyond, beyond[:8]]).astype(np.int32).cumsum(0)
            run = np.concatenate([np.zeros((1,) + v.shape, np.int32), run])
            ok |= ((run[9:] - run[:-9]) == 9).any(0)
        return ok
    lo = np.full(v.shape, -256, np.int32)                           # a corner at t = -256 always: every difference is > -256
    hi = np.full(v.shape, 255, np.int32)                            # never at t = 255
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ok = corner_at(mid)
        lo = np.where(ok, mid, lo); hi = np.where(ok, hi, mid)
    out = np.full((h, w), -1000, np.int32)
    out[3:h - 3, 3:w - 3] = lo
    return out


# ------------------------------------------------------------------------------------------------------------------------ BRIEF half-way roundings
def rotation(oracle, angle_deg):
    """(cos, sin) as computeOrbDescriptor has them: f32 angle * f32 pi/180, then the shared sin / cos"""
    rad = np.float32(angle_deg) * np.float32(np.pi / 180)
    s, c = oracle.sincos(float(rad))
    return np.float32(c), np.float32(s)


def brief_coordinates(pattern, a, b):
    """the 512 rotated pattern points before rounding, in f32 with every product and sum rounded on its own: (row, col) each (512,)"""
    P = np.asarray(pattern, np.int8).reshape(512, 2).astype(np.float32)
    x, y = P[:, 0], P[:, 1]
    a, b = np.float32(a), np.float32(b)
    return (x * b) + (y * a), (x * a) - (y * b)


def halfway(v):
    """coordinates exactly half-way between two integers"""
    return np.abs(v - np.trunc(v)) == np.float32(0.5)


def brief_numpy(blurred, x, y, row, col):
    """256 bits from rounded sample coordinates (512,) int: t(2i) < t(2i + 1), bit i % 8 of byte i // 8"""
    t = blurred[y + row, x + col].astype(np.int32)
    return np.packbits((t[0::2] < t[1::2]).astype(np.uint8), bitorder="little")


TIE_SLOTS = ("r0", "c0", "r1", "c1")                   # row / column of the first and of the second point of a test


def tie_report(oracle, pattern, blurred, x, y, angle_deg):
    """(half-way coordinates of the key-point, those whose other rounding changes a descriptor bit, the numpy descriptor, and for each of the
    latter (slot of TIE_SLOTS, whether rounding half away from zero would take the other pixel))"""
    a, b = rotation(oracle, angle_deg)
    r, c = brief_coordinates(pattern, a, b)
    ri, ci = np.rint(r).astype(np.int64), np.rint(c).astype(np.int64)              # half to even, as cvRound and __float2int_rn
    base = brief_numpy(blurred, x, y, ri, ci)
    ties, detail = 0, []
    for arr, rounded, is_row in ((r, ri, True), (c, ci, False)):
        for i in np.nonzero(halfway(arr))[0]:
            ties += 1
            other = rounded.copy()
            other[i] = rounded[i] + (1 if arr[i] > rounded[i] else -1)
            d = brief_numpy(blurred, x, y, other, ci) if is_row else brief_numpy(blurred, x, y, ri, other)
            if not np.array_equal(d, base):
                detail.append((("r" if is_row else "c") + str(i % 2), bool(abs(other[i]) > abs(rounded[i]))))
    return ties, len(detail), base, detail


def tie_background(seed):
    """seeded low-contrast texture: smooth waves and +-12 of noise around 110, so that neighbouring blurred pixels differ"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = 110 + 25 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + rng.integers(-12, 13, (H, W))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


TIE_POSITIONS = [(40, 40, "right"), (100, 40, "down"), (160, 40, "left"), (40, 110, "up"), (100, 110, "right"), (160, 110, "left")]


def tie_image(seed, length, bar, along, side, delta):
    """the stamp family of the search: six bars of `length` and brightness `bar` (end pixel 250) on tie_background(seed), each with one satellite
    pixel (along, side, delta)"""
    img = tie_background(seed)
    for x, y, d in TIE_POSITIONS:
        stamp(img, x, y, d, bar, 250, length=length, sat=(along, side, delta))
    return img


TIE_NFEATURES = 150
# (seed, bar length, bar brightness, satellite along, side, delta): images of the search (search_tie_stamps; 58 of 40 000 stamps had a half-way
# coordinate whose other rounding changes a descriptor bit), chosen so that each of the four roundings of a test (TIE_SLOTS) meets at least two such
# coordinates on which half-to-even and half-away-from-zero disagree, and one on which they agree (truncation still differs there);
# tests/test_orb_cases.py recounts them
TIE_STAMPS = [(346, 9, 186, 6, -1, -27), (969, 24, 203, 7, 1, -55), (14, 9, 186, 4, 1, -9), (629, 24, 192, 4, -1, -14), (967, 20, 213, 5, -1, 0),
              (712, 18, 207, 5, -1, -14), (716, 10, 216, 7, -1, -54), (848, 23, 237, 4, -1, -20), (341, 23, 223, 5, -1, -25)]
# k: angles tie_angle(k) with the most half-way coordinates among the 1024 of a descriptor (search_tie_angles): of the 65 536 multiples of
# 360 / 65536 only 7 have any (20 coordinates in all), so the list holds the best 4 of those (4 coordinates each, k % 16 == 0) and the best 28
# of the 2^20 multiples of 360 / 2^20 (229 angles have any; 5 to 8 coordinates each)
TIE_ANGLES = [13303, 57732, 75456, 131653, 138610, 186668, 197963, 206247, 222703, 234814, 319876, 383179, 389349, 448812, 460107, 468391, 496958, 507034, 556207, 582020, 595312, 599744, 655941, 710956, 725644, 727602, 844081, 861888, 918085, 925042, 984395, 1041469]


TIE_ANGLE_STEPS = 1 << 20


def tie_angle(k):
    """k * 360 / 2^20 rounded to f32; the multiples of 16 are the 65 536 multiples of 360 / 65536, which are exact"""
    return np.float32(k * 360.0 / TIE_ANGLE_STEPS)


def brief_ties():
    return [Case(f"brief_ties[{i}]", "ties", tie_image(*p), TIE_NFEATURES, 3, stamp=p) for i, p in enumerate(TIE_STAMPS)]


def tie_angle_keypoints(kp_dtype, nlevels=3, scale=1.2):
    """CalcDescriptors takes the caller's angle: every angle of TIE_ANGLES at three positions of a noise image, levels 0 .. nlevels - 1 in turn"""
    img = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)      # full-range noise: neighbouring blurred pixels differ most often
    k = np.zeros(3 * len(TIE_ANGLES), kp_dtype)
    for i in range(len(k)):
        lvl = i % nlevels
        s = np.float32(scale) ** lvl
        k[i]["x"], k[i]["y"] = np.float32(40 + (i * 17) % 120), np.float32(40 + (i * 29) % 80)
        k[i]["angle"] = tie_angle(TIE_ANGLES[i // 3])
        k[i]["octave"], k[i]["size"], k[i]["response"], k[i]["class_id"] = lvl, 31 * s, -1, i
    return img, k


def search_tie_angles(oracle, keep=32, ks=range(TIE_ANGLE_STEPS)):
    """half-way coordinates of every angle tie_angle(k): -> (the `keep` angles with the most, {k: count} of all that have any)"""
    P = oracle.pattern().reshape(512, 2).astype(np.float32)
    x, y = P[:, 0][None], P[:, 1][None]
    found = {}
    ks = list(ks)
    for i in range(0, len(ks), 4096):
        chunk = ks[i:i + 4096]
        ab = np.array([rotation(oracle, tie_angle(k)) for k in chunk], np.float32)
        a, b = ab[:, 0:1], ab[:, 1:2]
        n = halfway((x * b) + (y * a)).sum(1) + halfway((x * a) - (y * b)).sum(1)
        for j in np.nonzero(n)[0]:
            found[chunk[j]] = int(n[j])
    best = sorted(found, key=lambda k: (-found[k], k))[:keep]
    return sorted(best), found


def count_image_ties(oracle, case):
    """(half-way coordinates, those that flip a bit, their (slot, half-away differs) list) over all key-points the oracle finds in the case's image"""
    p = case.params(oracle)
    kps, desc = oracle.detect_and_compute(p, case.img)
    pyr = oracle.pyramid(p, case.img)
    blur = [oracle.blur7(l, 0) for l in pyr]
    pat = oracle.pattern()
    sc = oracle.orb_tables(p)[0]
    ties, detail = 0, []
    for k, d in zip(kps, desc):
        l = int(k["octave"])
        x, y = (int(k["x"]), int(k["y"])) if l == 0 else (int(np.rint(k["x"] / sc[l])), int(np.rint(k["y"] / sc[l])))
        t, f, mine, det = tie_report(oracle, pat, blur[l], x, y, k["angle"])
        if not np.array_equal(mine, d):                               # levels above 0: x * scale / scale may not round back; skip those
            continue
        ties += t; detail += det
    return ties, len(detail), detail


def search_tie_stamps(oracle, trials=4000, seed=1):
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(trials):
        p = (int(rng.integers(0, 1000)), int(rng.integers(8, 25)), int(rng.integers(180, 241)), int(rng.integers(4, 8)),
             int(rng.choice([-1, 1])), int(rng.integers(-60, 11)))
        c = Case("search", "ties", tie_image(*p), TIE_NFEATURES, 3)
        t, f, detail = count_image_ties(oracle, c)
        if f:
            found.append((f, t, p, detail))
    found.sort(key=lambda r: (-r[0], r[2]))
    return found


ALL_BUILDERS = (threshold_ladder, fallback_cells, arcs, extremes, plateaus, seams, octree_split_lines, octree_budgets, octree_equal_responses,
                octree_equal_sizes, octree_deep, octree_wide, axis_angles, brief_ties)


def all_cases():
    return [c for b in ALL_BUILDERS for c in b()]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    from pyoracle import Oracle
    orc = Oracle()
    ks, count = search_tie_angles(orc)
    print("TIE_ANGLES =", ks, "# half-way coordinates:", [count[k] for k in ks], "of", sum(count.values()), "at", len(count), "angles")
    for f, t, p, detail in search_tie_stamps(orc, trials=40000)[:40]:
        print(f"    {p},  # {t} half-way, {f} flip a bit: {detail}")
