"""Hand-made inputs of the 256-bit Hamming matcher and the stereo triangulation (csrc/match_tri.hip) at small sizes, for what uniform random
bytes and noisy KITTI projections never produce: ties at every register, half-wave, chunk and wave-group position, every distance 0 .. 256,
counts outside [0, cap], the two acceptance gates of the triangulation at their thresholds, non-finite key-points, match indices outside the
slots.  No GPU here.  tests/test_match_tri_cases.py proves on the oracle alone that every case reaches the regime it is named for;
tests/test_gpu_match_edges.py runs the device on the same inputs.

A Hamming builder returns (q, nq, t, nt, expected_idx, expected_dist): q, t are (B, cap, 32) uint8 (EVERY slot holds readable bytes, whatever
the counts say), nq, nt (B,) int32 as they are handed to the device, expected_* (B, cap) int32 in closed form with SENTINEL in every slot the
call must leave alone.  Train rows of a 32-row chunk sit in the kernel as: lanes 0-31 rows 0-3, 8-11, 16-19, 24-27, lanes 32-63 the others;
the one-pair form gives chunk c to wave group c % 4."""
import numpy as np

SENTINEL = -7
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


# ------------------------------------------------------------------------------------------------------------------------ Hamming
def popcount(a, b):
    """Hamming distance of 32-byte rows (broadcast)"""
    return np.unpackbits(np.bitwise_xor(a, b), axis=-1).sum(-1).astype(np.int32)


def masks(rng, ks):
    """one 32-byte mask per entry of ks with exactly that many bits set, at random positions over all 256"""
    ks = np.asarray(ks).reshape(-1)
    rank = rng.random((len(ks), 256)).argsort(1).argsort(1)
    return np.packbits((rank < ks[:, None]).astype(np.uint8), axis=1)


def brute(q, t):
    """first-minimum brute force in numpy (not the oracle's code): (idx, dist), -1 / -1 without train rows"""
    if len(t) == 0:
        return np.full(len(q), -1, np.int32), np.full(len(q), -1, np.int32)
    d = popcount(q[:, None, :], t[None, :, :])
    i = d.argmin(1).astype(np.int32)
    return i, d[np.arange(len(q)), i]


def clamp(n, cap):
    return int(min(max(int(n), 0), cap))


def _blank(rng, B, cap):
    q = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8); t = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    return q, t, np.full((B, cap), SENTINEL, np.int32), np.full((B, cap), SENTINEL, np.int32)


def _queries(rng, D, n):
    """n queries within 0 .. 3 bits of D -> (rows, distances to D)"""
    k = np.arange(n) % 4
    return D ^ masks(rng, k), k.astype(np.int32)


SUFFIX_NT = 161                                        # five full chunks and a tail of one row; chunk 4 is group 0's second step


def suffix_ties(seed=1, nt=SUFFIX_NT, cap=168):
    """item s: rows s .. nt-1 are ONE descriptor within 3 bits of every query, rows 0 .. s-1 are random (~128 bits away): the first of many tied
    rows at every position.  Expected index s."""
    rng = np.random.default_rng(seed)
    q, t, ei, ed = _blank(rng, nt, cap)
    nq = (33 + np.arange(nt) % 8).astype(np.int32)
    for s in range(nt):
        D = rng.integers(0, 256, 32, dtype=np.uint8)
        q[s, :nq[s]], ed[s, :nq[s]] = _queries(rng, D, nq[s])
        t[s, s:nt] = D
        ei[s, :nq[s]] = s
    return q, nq, t, np.full(nt, nt, np.int32), ei, ed


# (tied rows, nt): the expected index is the first of them
PAIR_TIES = [((0, 1), 161), ((3, 4), 161), ((7, 8), 140), ((31, 32), 161), ((127, 128), 161), ((5, 37), 161), ((33, 161), 170),
             ((40, 130), 161), ((100, 128), 129), ((10, 169), 170), ((160, 169), 170), ((3, 4, 36), 161), ((40, 100, 130), 161),
             ((0, 31, 160), 161), ((7, 8, 128), 129), ((64, 96, 175), 176)]


def pair_ties(seed=2, cap=176):
    """exactly two (or three) identical nearest rows among random ones"""
    rng = np.random.default_rng(seed)
    B = len(PAIR_TIES)
    q, t, ei, ed = _blank(rng, B, cap)
    nq = (33 + np.arange(B) % 8).astype(np.int32)
    for b, (rows, _) in enumerate(PAIR_TIES):
        D = rng.integers(0, 256, 32, dtype=np.uint8)
        q[b, :nq[b]], ed[b, :nq[b]] = _queries(rng, D, nq[b])
        t[b, list(rows)] = D
        ei[b, :nq[b]] = rows[0]
    return q, nq, t, np.array([n for _, n in PAIR_TIES], np.int32), ei, ed


LADDER_NT = (37, 70, 101, 161)                         # none a multiple of 32
LADDER_NQ = (1, 33, 40, 7)


def distance_ladder(seed=3, cap=168):
    """item m = 0 .. 256: every train row is q ^ mask with popcount(mask) >= m, exactly one row has m (the answer), for m < 256 a row with m + 1
    sits at a lower index; every query of the item is q.  The slots past nt hold q itself: a row the kernel must not see.  Item 257: 70 rows, all
    ~q (every distance 256): index 0."""
    rng = np.random.default_rng(seed)
    B = 258
    q, t, ei, ed = _blank(rng, B, cap)
    nq = np.zeros(B, np.int32); nt = np.zeros(B, np.int32)
    for m in range(B):
        q0 = rng.integers(0, 256, 32, dtype=np.uint8)
        nq[m] = LADDER_NQ[m % 4]
        q[m, :nq[m]] = q0
        if m >= 256:
            nt[m] = 1 if m == 256 else 70
            t[m, :nt[m]] = ~q0
            ei[m, :nq[m]] = 0; ed[m, :nq[m]] = 256
        else:
            n = nt[m] = LADDER_NT[m % 4]
            pos = n - 1 if m % 5 == 0 else int(rng.integers(1, n))
            k = rng.integers(m + 1, 257, n)
            k[pos] = m; k[int(rng.integers(0, pos))] = m + 1
            t[m, :n] = q0 ^ masks(rng, k)
            ei[m, :nq[m]] = pos; ed[m, :nq[m]] = m
        t[m, nt[m]:] = q0
    return q, nq, t, nt, ei, ed


def count_edges(seed=4, cap=40):
    """counts above cap act as cap, a negative nq writes nothing, a negative nt with a positive nq gives index -1 and distance -1"""
    rng = np.random.default_rng(seed)
    spec = [(40, 33), (cap + 1, 20), (17, cap + 1), (2 * cap, 2 * cap), (I32_MAX, 5), (9, I32_MAX), (I32_MAX, I32_MAX), (-1, 30), (30, -1),
            (I32_MIN, 12), (12, I32_MIN), (-1, -1), (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (0, 5), (5, 0), (1, 1), (33, 40), (cap + 1, -1)]
    B = len(spec)
    q, t, ei, ed = _blank(rng, B, cap)
    for b, (a, c) in enumerate(spec):
        n, m = clamp(a, cap), clamp(c, cap)
        if c > cap and n > 0:
            t[b, cap - 1] = q[b, 0]                    # the last row a clamped count still covers is query 0's answer
        ei[b, :n], ed[b, :n] = brute(q[b, :n], t[b, :m])
    return q, np.array([s[0] for s in spec], np.int32), t, np.array([s[1] for s in spec], np.int32), ei, ed


HAMMING_BUILDERS = {"suffix_ties": suffix_ties, "pair_ties": pair_ties, "distance_ladder": distance_ladder, "count_edges": count_edges}


# ------------------------------------------------------------------------------------------------------------------------ triangulation
IMG_W, IMG_H = 1241, 376
POSITIONS = [(620.5, 187.75), (0.0, 0.0), (1240.0, 375.0), (-300.25, -200.5), (10000.5, 9000.25)]          # centre, corners, outside
DISPARITIES = [s * 2.0 ** k for k in range(-7, 10) for s in (1, -1)]
DY_AROUND = (0.5, 0.9, 0.99, 0.999, 1.001, 1.01, 1.1, 2.0)             # multiples of the offset at which the reference's ratio crosses 1e-2
RATIO_GATE = 1e-2
# Disparity exactly 0: the null vector's w is rounding noise and the sign of z with it.  The nine evaluations show that for most left points but
# not for all (at pixel (0, 0) of the second intrinsics set eight of them return the unperturbed bits); one pixel beside each position they
# disagree for every set, which tests/test_match_tri_cases.py asserts.
ZERO_AT = (1.0, 1.0)


def intrinsics(synth):
    """name -> (fx, fy, cx, cy, baseline)"""
    K = synth.KITTI00
    k = (K["fx"], K["fy"], K["cx"], K["cy"])
    return {"kitti00": k + (K["bf"] / K["fx"],), "anisotropic_off_centre": (458.654, 912.3, -150.5, 1290.25, 0.11),
            "baseline_5cm": k + (0.05,), "baseline_5m": k + (5.0,)}


def _poses(baseline):
    return np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, -baseline, 0, 1, 0, 0, 0, 0, 1, 0]], np.float64)


def normalised(K5, x4):
    """pixel (xl, yl, xr, yr) -> camera coordinates, as Camera::pixel2camera does in f64"""
    fx, fy, cx, cy = K5[:4]
    x4 = np.asarray(x4, np.float64)
    return np.array([(x4[0] - cx) / fx, (x4[1] - cy) / fy, (x4[2] - cx) / fx, (x4[3] - cy) / fy])


def solve(oracle, poses, u4):
    """the oracle's general f64 entry on one normalised stereo observation -> (xyz, ratio, accepted)"""
    xyz, r = oracle.triangulate(poses, np.array([[u4[0], u4[1], 1.0], [u4[2], u4[3], 1.0]]))
    return xyz, r, bool(r < RATIO_GATE and xyz[2] > 0)


def classify(oracle, K5, xl, yl, xr, yr):
    """Per point: the reference's decision, whether it survives a one-ulp move of each normalised coordinate in each direction (nine evaluations
    agree = stable), its xyz and ratio, and the largest move of xyz over the nine (per component)."""
    poses = _poses(K5[4])
    n = len(xl)
    out = {"ok": np.zeros(n, bool), "stable": np.zeros(n, bool), "xyz": np.zeros((n, 3)), "ratio": np.zeros(n), "spread": np.zeros((n, 3))}
    with np.errstate(all="ignore"):
        for i in range(n):
            u = normalised(K5, (xl[i], yl[i], xr[i], yr[i]))
            xyz, r, ok = solve(oracle, poses, u)
            same, spread = True, np.zeros(3)
            for c in range(4):
                for to in (np.inf, -np.inf):
                    v = u.copy(); v[c] = np.nextafter(u[c], to)
                    x2, _, ok2 = solve(oracle, poses, v)
                    same &= ok2 == ok
                    spread = np.fmax(spread, np.abs(x2 - xyz))
            out["ok"][i], out["stable"][i], out["xyz"][i], out["ratio"][i], out["spread"][i] = ok, same, xyz, r, spread
    return out


def crossing(oracle, K5, pos, disp, sign):
    """the vertical offset (px, of the given sign) at which the reference's ratio crosses the gate for this point and disparity: geometric
    bisection between 1e-3 and 1e5 px, None if both ends lie on one side"""
    poses = _poses(K5[4])
    xl, yl = np.float32(pos[0]), np.float32(pos[1])
    xr = np.float32(xl - np.float32(disp))
    ratio = lambda dy: solve(oracle, poses, normalised(K5, (xl, yl, xr, np.float64(yl) + sign * dy)))[1]
    lo, hi = 1e-3, 1e5
    if not (ratio(lo) < RATIO_GATE <= ratio(hi)):
        return None
    for _ in range(26):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if ratio(mid) < RATIO_GATE else (lo, mid)
    return sign * np.sqrt(lo * hi)


_LADDERS = {}


def gate_ladder(oracle, synth, name):
    """disparities +-2^k, k = -7 .. 9, x vertical offsets around the reference's own gate crossing (found per point, disparity and sign), 0 and
    +-30 px, x five left points; plus disparity exactly 0 without vertical offset at every left point.  float32 pixels.  Built and classified
    once per process: {"xl", "yl", "xr", "yr", "K5", "disp", "dy", "ref" (classify's result)}."""
    if name in _LADDERS:
        return _LADDERS[name]
    K5 = intrinsics(synth)[name]
    rows = []
    for pos in POSITIONS:
        for d in DISPARITIES:
            dys = [0.0, 30.0, -30.0]
            for sign in (1.0, -1.0):
                c = crossing(oracle, K5, pos, d, sign)
                dys += [m * c for m in DY_AROUND] if c is not None else []
            rows += [(pos[0], pos[1], d, dy) for dy in dys]
        rows.append((pos[0] + ZERO_AT[0], pos[1] + ZERO_AT[1], 0.0, 0.0))
    a = np.array(rows, np.float64)
    xl, yl = a[:, 0].astype(np.float32), a[:, 1].astype(np.float32)
    xr = (xl - a[:, 2].astype(np.float32)).astype(np.float32)
    yr = (yl.astype(np.float64) + a[:, 3]).astype(np.float32)
    L = {"name": name, "xl": xl, "yl": yl, "xr": xr, "yr": yr, "K5": K5, "disp": a[:, 2], "dy": a[:, 3]}
    L["ref"] = classify(oracle, K5, xl, yl, xr, yr)
    _LADDERS[name] = L
    return L


BAD_VALUES = (np.nan, np.inf, -np.inf, 3e38, -3e38)
NONFINITE_N = 2 * 256 + 77                             # two full blocks and a partial one


def nonfinite(synth, seed=5):
    """benign KITTI projections with each bad value in each of the four coordinates in turn, in all four waves of the first block and in the
    partial last block -> {"good": (xl, yl, xr, yr) f32, "bad": the same with the values planted, "where": indices, "nonfinite": those that are
    NaN or inf (3e38 is a finite float), "K5"}"""
    K5 = intrinsics(synth)["kitti00"]
    rng = np.random.default_rng(seed)
    n = NONFINITE_N
    Z = rng.uniform(3, 80, n); X = rng.uniform(-15, 15, n); Y = rng.uniform(-3, 3, n)
    good = np.stack([K5[0] * X / Z + K5[2], K5[1] * Y / Z + K5[3], K5[0] * (X - K5[4]) / Z + K5[2], K5[1] * Y / Z + K5[3] + rng.normal(0, 0.3, n)]).astype(np.float32)
    bad = good.copy()
    where, nonfin = [], []
    for k, (v, c) in enumerate((v, c) for v in BAD_VALUES for c in range(4)):
        for i in [w * 64 + 3 * k + 1 for w in range(4)] + [512 + 3 * k + 2]:
            bad[c, i] = v
            where.append(i)
            if not np.isfinite(v):
                nonfin.append(i)
    return {"good": tuple(good), "bad": tuple(bad), "where": np.array(where), "nonfinite": np.array(nonfin), "K5": K5}


BAD_MATCH_CAP = 40


def bad_matches(synth, seed=6, cap=BAD_MATCH_CAP):
    """key-point form: items whose match lists hold -1, cap, cap + 7, INT32_MAX and INT32_MIN beside valid indices, every unused field of the
    28-byte records filled with NaN or garbage bits, nl above cap and negative in some items -> {"kl", "kr" (B, cap) records, "kl_clean",
    "kr_clean" (the same x, y, zeros elsewhere), "match" (B, cap), "nl" (B,), "K5"}"""
    K5 = intrinsics(synth)["kitti00"]
    rng = np.random.default_rng(seed)
    nl = np.array([cap, 33, cap + 1, I32_MAX, -1, I32_MIN, 0, 2 * cap, 17], np.int32)
    B = len(nl)
    Z = rng.uniform(3, 80, (B, cap)); X = rng.uniform(-15, 15, (B, cap)); Y = rng.uniform(-3, 3, (B, cap))
    kl = np.zeros((B, cap), KP); kr = np.zeros((B, cap), KP)
    match = np.stack([rng.permutation(cap) for _ in range(B)]).astype(np.int32)
    kl["x"] = K5[0] * X / Z + K5[2]; kl["y"] = K5[1] * Y / Z + K5[3]
    for b in range(B):                                 # right key-point of left i sits in slot match[b, i]
        kr["x"][b, match[b]] = K5[0] * (X[b] - K5[4]) / Z[b] + K5[2]
        kr["y"][b, match[b]] = kl["y"][b] + rng.normal(0, 0.3, cap)
    kl_clean, kr_clean = kl.copy(), kr.copy()
    for k in (kl, kr):
        bits = rng.integers(0, 2 ** 32, (B, cap, 5), dtype=np.uint64).astype(np.uint32)
        bits[:, 0::3, :3] = np.float32(np.nan).view(np.uint32)
        k["size"] = bits[..., 0].view(np.float32); k["angle"] = bits[..., 1].view(np.float32); k["response"] = bits[..., 2].view(np.float32)
        k["octave"] = bits[..., 3].view(np.int32); k["class_id"] = bits[..., 4].view(np.int32)
    bad = [-1, cap, cap + 7, I32_MAX, I32_MIN]
    for b in range(B):
        for k, v in enumerate(bad):
            match[b, (3 * k + 2 * b + 1) % cap] = v    # each between valid neighbours; positions differ per item
    return {"kl": kl, "kr": kr, "kl_clean": kl_clean, "kr_clean": kr_clean, "match": match, "nl": nl, "K5": K5, "cap": cap}


def bad_matches_expected(oracle, c):
    """(xyz (B, cap, 3), ok (B, cap), written (B, cap)) by the rule of the header, valid matches through the oracle"""
    B, cap = c["match"].shape
    xyz = np.zeros((B, cap, 3)); ok = np.zeros((B, cap), bool); written = np.zeros((B, cap), bool)
    for b in range(B):
        n = clamp(c["nl"][b], cap)
        written[b, :n] = True
        m = c["match"][b, :n]
        v = (m >= 0) & (m < cap)
        i = np.flatnonzero(v)
        if len(i):
            xyz[b, i], ok[b, i] = oracle.triangulate_stereo(c["kl"]["x"][b, i], c["kl"]["y"][b, i], c["kr"]["x"][b, m[i]], c["kr"]["y"][b, m[i]], *c["K5"])
    return xyz, ok, written
