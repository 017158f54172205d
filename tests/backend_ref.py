"""Backend::OptimizeActiveMap (reference src/backend.cpp:126-266) and the Map calls it makes (src/map.cpp:126-175) as a literal walk over Python
containers, with the solve passed in as a function; a packer from those containers to the device tables of myslam_backend_optimize_batch
(include/myslam_hip.h); and make_map, synthetic active maps built on synth.ba_problem with every kind of row the tables can hold.  Test helper, no GPU."""
import copy

import numpy as np

ACTIVE, OUTLIER = 1, 2                      # MYSLAM_BACKEND_OBS_*
DONE, EMPTY, INVALID = 0, 1, -1             # MYSLAM_BACKEND_DONE / _EMPTY, MYSLAM_ERR_INVALID
CHI2_TH = 5.991


class Obs:                                  # a Feature as a map point's observation lists see it
    __slots__ = ("kf", "u", "v", "outlier", "tag")

    def __init__(self, kf, u, v, outlier=False, tag=0):
        self.kf, self.u, self.v, self.outlier, self.tag = int(kf), np.float32(u), np.float32(v), bool(outlier), int(tag)


class MapPoint:
    __slots__ = ("id", "pos", "outlier", "obs", "active_obs")

    def __init__(self, mp_id, pos, outlier=False):
        self.id, self.pos, self.outlier = int(mp_id), np.array(pos, float), bool(outlier)
        self.obs, self.active_obs = [], []  # GetObservations() / GetActiveObservations(): the same Obs objects


class Map:
    def __init__(self):
        self.kfs = {}                       # GetActiveKeyFrames(): mnKFId -> pose7 (Tcw)
        self.mps = {}                       # GetActiveMapPoints(): mnId -> MapPoint
        self.outlier_list = []              # _mlistOutlierMapPoints

    def clone(self):
        return copy.deepcopy(self)


def _is_in(lst, o):
    return any(g is o for g in lst)


def _drop(lst, o):
    for i, g in enumerate(lst):
        if g is o:
            del lst[i]
            return


def rows_of(m):
    """The observation table's rows in table order: [(map-point row, MapPoint, Obs)]"""
    return [(i, m.mps[mid], o) for i, mid in enumerate(sorted(m.mps)) for o in m.mps[mid].obs]


def validate(m):
    """What the device refuses with MYSLAM_ERR_INVALID and a Map can express (chain.py:589, the assert of backend.cpp:187)"""
    for mp in m.mps.values():
        if not mp.outlier and not mp.obs:
            return False
        if any(o.kf not in m.kfs for o in mp.active_obs) or any(not _is_in(mp.obs, o) for o in mp.active_obs):
            return False
    return True


def flatten(m):
    """backend.cpp:139-206 with g2o's vertex order (ids ascending) -> flat arrays in myslam_ba_flatten_window's form, edge_src = TABLE row, plus the
    (MapPoint, Obs) of every edge and the MapPoint of every landmark slot"""
    kf_ids = sorted(m.kfs)
    kf_slot = {k: i for i, k in enumerate(kf_ids)}                        # :139-150
    row = {}
    for r, (_, _, o) in enumerate(rows_of(m)):
        row[id(o)] = r
    pt_src, fixed, ep, el, eo, es, edge_objs, slot_mps = [], [], [], [], [], [], [], []
    for i, mid in enumerate(sorted(m.mps)):                                 # :161
        mp = m.mps[mid]
        if mp.outlier:                                                      # :163
            continue
        is_fixed = mp.obs[0].kf not in m.kfs                                # :175
        edges = []
        for o in mp.active_obs:                                             # :183
            assert o.kf in m.kfs                                            # :187
            if o.outlier:                                                   # :189
                continue
            edges.append(o)
        if not edges:                                                       # a vertex without an edge is never activated
            continue
        j = len(pt_src)
        pt_src.append(i); fixed.append(1 if is_fixed else 0); slot_mps.append(mp)
        for o in edges:
            ep.append(kf_slot[o.kf]); el.append(j); eo.append((np.float64(o.u), np.float64(o.v))); es.append(row[id(o)]); edge_objs.append((mp, o))
    return dict(pose_src=np.arange(len(kf_ids), dtype=np.int32), pt_src=np.array(pt_src, np.int32), fixed=np.array(fixed, np.uint8),
                edge_pose=np.array(ep, np.int32), edge_pt=np.array(el, np.int32), edge_obs=np.array(eo, np.float64).reshape(-1, 2),
                edge_src=np.array(es, np.int32)), edge_objs, slot_mps


def walk(m, solve):
    """Backend::OptimizeActiveMap on `m` (changed in place).  solve(poses, pts, edge_pose, edge_pt, edge_obs, fixed) -> (poses, pts, chi2, outlier flags,
    rounds, outlier count): backend.cpp:208-232 and the test `chi2 > chi2_th` of :237.  Returns the reports of myslam_backend_optimize_batch by INPUT row,
    and left_pos: INPUT row -> the optimised position of every map point that had a vertex and left the active set alive."""
    rows = rows_of(m)
    n_mp, n_obs = len(m.mps), len(rows)
    rep = dict(status=DONE, obs_report=np.zeros(n_obs, np.uint8), mp_report=np.zeros(n_mp, np.uint8), new_outlier=[], obs_chi2=np.zeros(n_obs),
               rounds=0, n_outlier_edges=0, flat=None, left_pos={})
    if not validate(m):
        rep["status"] = INVALID
        return rep
    flat, edge_objs, slot_mps = flatten(m)
    if len(edge_objs) == 0:                                                 # chain.py:596
        rep["status"] = EMPTY
        return rep
    rep["flat"] = flat
    row_of_obs = {id(o): r for r, (_, _, o) in enumerate(rows)}
    row_of_mp = {mid: i for i, mid in enumerate(sorted(m.mps))}
    kf_ids = sorted(m.kfs)
    poses = np.stack([m.kfs[k] for k in kf_ids]); pts = np.stack([mp.pos for mp in slot_mps])
    p2, x2, chi, out, rounds, nout = solve(poses, pts, flat["edge_pose"], flat["edge_pt"], flat["edge_obs"], flat["fixed"])
    rep["rounds"], rep["n_outlier_edges"] = int(rounds), int(nout)
    rep["obs_chi2"][:] = -1.0
    for e, (mp, o) in enumerate(edge_objs):                                 # :236-251
        rep["obs_chi2"][row_of_obs[id(o)]] = chi[e]
        if out[e]:
            o.outlier = True
            _drop(mp.active_obs, o)                                         # RemoveActiveObservation
            _drop(mp.obs, o)                                                # RemoveObservation
            rep["obs_report"][row_of_obs[id(o)]] = 1
            if not mp.obs:                                                  # :243-246
                mp.outlier = True
                m.outlier_list.append(mp.id)
                rep["new_outlier"].append(row_of_mp[mp.id])
        else:
            o.outlier = False
    for i, k in enumerate(kf_ids):                                          # :256-258
        m.kfs[k] = np.array(p2[i], float)
    for j, mp in enumerate(slot_mps):                                       # :259-261
        mp.pos = np.array(x2[j], float)
    gone = []
    for mid in m.outlier_list:                                              # RemoveAllOutlierMapPoints, map.cpp:166-175
        mp = m.mps.pop(mid, None)
        if mp is not None:
            rep["mp_report"][row_of_mp[mid]] = 2
            gone.append(mp)
    m.outlier_list = []
    for mid in [k for k, mp in m.mps.items() if not mp.active_obs]:        # RemoveOldActiveMapPoints, map.cpp:126-140
        rep["mp_report"][row_of_mp[mid]] = 1
        gone.append(m.mps.pop(mid))
        if _is_in(slot_mps, gone[-1]):                                      # :259-261 came first: the point leaves with its optimised position, which
            rep["left_pos"][row_of_mp[mid]] = gone[-1].pos.copy()           # the tables no longer hold (INPUT row -> position: myslam_map_attach_solve)
    for mp in gone:
        for o in mp.obs:
            rep["obs_report"][row_of_obs[id(o)]] = 2
    return rep


def pack(m):
    """One map's tables, unpadded, in the layout of myslam_backend_optimize_batch"""
    kf_ids = sorted(m.kfs); mp_ids = sorted(m.mps)
    kf_row = {k: i for i, k in enumerate(kf_ids)}
    rows = rows_of(m)
    for mp in m.mps.values():                                               # the caller's obligation: ACTIVE rows in GetActiveObservations() order
        act = [o for o in mp.obs if _is_in(mp.active_obs, o)]
        assert len(act) == len(mp.active_obs) and all(a is b for a, b in zip(act, mp.active_obs))
    return dict(
        kf_id=np.array(kf_ids, np.int64), kf_pose=np.array([m.kfs[k] for k in kf_ids], np.float64).reshape(-1, 7),
        mp_id=np.array(mp_ids, np.int64), mp_pos=np.array([m.mps[i].pos for i in mp_ids], np.float64).reshape(-1, 3),
        mp_outlier=np.array([m.mps[i].outlier for i in mp_ids], np.uint8),
        obs_mp=np.array([r[0] for r in rows], np.int32), obs_kf=np.array([kf_row.get(o.kf, -1) for _, _, o in rows], np.int32),
        obs_flags=np.array([(ACTIVE if _is_in(mp.active_obs, o) else 0) | (OUTLIER if o.outlier else 0) for _, mp, o in rows], np.uint8),
        obs_uv=np.array([(o.u, o.v) for _, _, o in rows], np.float32).reshape(-1, 2), obs_tag=np.array([o.tag for _, _, o in rows], np.int32))


TABLES = ("kf_id", "kf_pose", "mp_id", "mp_pos", "mp_outlier", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag")
_COUNT_OF = dict(kf_id="n_kf", kf_pose="n_kf", mp_id="n_mp", mp_pos="n_mp", mp_outlier="n_mp", obs_mp="n_obs", obs_kf="n_obs", obs_flags="n_obs",
                 obs_uv="n_obs", obs_tag="n_obs")
_FILL = dict(kf_id=-77, kf_pose=-7.5, mp_id=-88, mp_pos=-8.5, mp_outlier=0xEE, obs_mp=-99, obs_kf=-98, obs_flags=0xDD, obs_uv=-9.5, obs_tag=-97)


def pack_batch(maps, kf_cap, mp_cap, obs_cap):
    """Strided tables of a batch (numpy), every slot from an item's count on filled with a sentinel, + the counts"""
    caps = dict(n_kf=kf_cap, n_mp=mp_cap, n_obs=obs_cap)
    items = [pack(m) for m in maps]
    out = {}
    for name in TABLES:
        proto = items[0][name]
        a = np.full((len(maps), caps[_COUNT_OF[name]]) + proto.shape[1:], _FILL[name], proto.dtype)
        for b, it in enumerate(items):
            assert len(it[name]) <= a.shape[1], (name, len(it[name]), a.shape[1])
            a[b, :len(it[name])] = it[name]
        out[name] = a
    for cnt, name in (("n_kf", "kf_id"), ("n_mp", "mp_id"), ("n_obs", "obs_mp")):
        out[cnt] = np.array([len(it[name]) for it in items], np.int32)
    return out


def host_flatten_args(m):
    """The arguments of api.ba_flatten_window (ids, the active observation lists) for a Map, and the table row of each of its observation rows"""
    mp_ids = sorted(m.mps)
    first = [(m.mps[i].obs[0].kf if m.mps[i].obs else 0) for i in mp_ids]
    act = [(r, mp, o) for r, (_, mp, o) in enumerate(rows_of(m)) if _is_in(mp.active_obs, o)]
    args = (np.array(sorted(m.kfs), np.uint64), np.array(mp_ids, np.uint64), np.array([m.mps[i].outlier for i in mp_ids], np.uint8),
            np.array(first, np.uint64), np.array([mp.id for _, mp, _ in act], np.uint64), np.array([o.kf for _, _, o in act], np.uint64),
            np.array([(o.u, o.v) for _, _, o in act], np.float32).reshape(-1, 2), np.array([o.outlier for _, _, o in act], np.uint8))
    return args, np.array([r for r, _, _ in act], np.int32)


def same_flat(table_flat, host_flat, active_rows):
    """a flat window whose edge_src names table rows against api.ba_flatten_window's (edge_src = index into the active rows): byte for byte"""
    for k in ("pose_src", "pt_src", "fixed", "edge_pose", "edge_pt", "edge_obs"):
        a, b = np.ascontiguousarray(table_flat[k]), np.ascontiguousarray(host_flat[k])
        if a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return False
    return np.array_equal(table_flat["edge_src"], active_rows[host_flat["edge_src"]]) and table_flat["edge_src"].dtype == np.int32


def make_map(synth, seed, n_kf=6, n_mp=60, outlier_frac=0.03, extras=True):
    """An active map over synth.ba_problem(seed, n_kf, n_mp): key-frame and map-point ids ascending with gaps, one ACTIVE row per edge, and (extras)
    non-active rows at the front (a first observer that left the window: the landmark is fixed), in the middle and at the end of segments (ACTIVE = 0
    rows of in-window key-frames, as LoopLocalFusion appends them), input outlier map points with and without rows, OUTLIER-bit rows, map points with
    no ACTIVE row, and two-observation landmarks whose second pixel is moved 30-50 px across the epipolar line, so that both edges fail and the
    point empties.  Returns (Map, K tuple, kinds: map-point id -> kind)."""
    poses, pts, ep, el, obs, fixed, K = synth.ba_problem(seed=seed, n_kf=n_kf, n_mp=n_mp, outlier_frac=outlier_frac)
    rng = np.random.default_rng([seed, 0xBACE])
    kf_ids = (20 + np.cumsum(rng.integers(1, 4, n_kf))).tolist()
    outside = [3, 7, 11]                                                    # key-frames that have left the window
    mp_ids = (100 + np.cumsum(rng.integers(1, 6, n_mp))).tolist()
    m = Map()
    for i, k in enumerate(kf_ids):
        m.kfs[k] = poses[i].copy()
    tag = [1000]
    kinds = {}

    def new_obs(kf, uv, outlier=False):
        tag[0] += int(rng.integers(1, 9))
        return Obs(kf, uv[0], uv[1], outlier, tag[0])

    for l in range(n_mp):
        mp = MapPoint(mp_ids[l], pts[l])
        m.mps[mp.id] = mp
        ks = np.nonzero(el == l)[0]
        r = rng.random() if extras else 1.0
        if len(ks) == 0 or r < 0.03:                                        # an old outlier without rows
            kind = "outlier_empty"
            mp.outlier = True
        elif r < 0.07:                                                      # an old outlier that still has rows
            kind = "outlier"
            mp.outlier = True
            for k in ks[:2]:
                o = new_obs(kf_ids[ep[k]], obs[k]); mp.obs.append(o); mp.active_obs.append(o)
        elif r < 0.12:                                                      # no ACTIVE row: it leaves the active set
            kind = "inactive"
            mp.obs.append(new_obs(outside[l % 3], obs[ks[0]]))
            if len(ks) > 1:
                mp.obs.append(new_obs(kf_ids[ep[ks[1]]], obs[ks[1]]))
        elif r < 0.19 and len(ks) >= 2:                                     # both edges fail: the point empties
            kind = "pair"
            c = np.array([K[2], K[3]])
            for n, k in enumerate(ks[[0, -1]]):
                uv = obs[k].copy()
                if n == 1:
                    d = uv - c
                    d = np.array([-d[1], d[0]]) / max(np.linalg.norm(d), 1e-9)      # across the (radial) epipolar line of a forward motion
                    uv += d * rng.uniform(30, 50) * rng.choice([-1, 1])
                o = new_obs(kf_ids[ep[k]], uv); mp.obs.append(o); mp.active_obs.append(o)
        else:
            kind = "fixed" if (fixed[l] and extras) else "normal"
            if kind == "fixed":                                             # front: the first observer has left the window
                mp.obs.append(new_obs(outside[l % 3], obs[ks[0]] + 1.5))
            mid = int(rng.integers(1, len(ks))) if (extras and len(ks) > 1 and rng.random() < 0.2) else -1
            for n, k in enumerate(ks):
                if n == mid:                                                # middle: a row of an in-window key-frame that is not active
                    mp.obs.append(new_obs(kf_ids[ep[k]], obs[k] + 0.75))
                o = new_obs(kf_ids[ep[k]], obs[k], outlier=extras and rng.random() < 0.05)
                mp.obs.append(o); mp.active_obs.append(o)
            if extras and rng.random() < 0.2:                               # end
                mp.obs.append(new_obs(kf_ids[ep[ks[-1]]], obs[ks[-1]] - 0.75))
        if mp.outlier:
            m.outlier_list.append(mp.id)
        kinds[mp.id] = kind
    return m, K, kinds
