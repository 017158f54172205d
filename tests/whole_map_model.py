"""The reference's whole Map as plain Python objects, and seeded random histories on it.  Test helper, no GPU.

WholeMap holds what src/map.cpp holds: every key-frame (with KeyFrame::mpLastKF / mRelativePoseToLastKF as they were when the key-frame was made), every
map point, the active subsets, the outlier list and the ids ever erased.  A MapPoint object persists after it leaves the active set, with its whole
GetObservations() list, so a point that comes back brings the rows it really had; tests/backend_ref.Map keeps the active part only.  The objects are
backend_ref's (Obs, MapPoint), so backend_ref.pack reads the active part (active_map()) and map_archive_ref.pack_chain / check_against_chain read the
model as they read <pkg>/chain.py's Chain (all_kfs, all_mps, outlier_mps, active_kfs, active_mps, last_kf, rel_to_last).  The calls are walks of the
reference's lines, written here a second time and independently of map_insert_ref.insert_walk, backend_ref.walk and map_archive_ref.update:
    insert_keyframe   src/frontend.cpp:263-264, :424-447, src/keyframe.cpp:34-50, src/map.cpp:17-48, :78-140, :159-164, src/mappoint.cpp:19-44
    optimize          src/backend.cpp:126-266 around the solve, src/map.cpp:126-140, :166-175, src/mappoint.cpp:34-56
The solve is not the model's: optimize() takes the outlier flag of every edge and the optimised numbers from outside.

history(seed, m, ...) is a generator of events on such a model.  Every structural decision comes from the seed, every number (poses, positions,
pixels) from the state of the model when the generator is resumed, so one seed gives one structure whether the numbers are the oracle's or the
device's.  Which observations the optimiser will remove is known by construction:

  A gross outlier (>= 60 px) pulls with the constant force of Huber's linear branch, and the inlier edges of the same landmark share that force: with
  fewer than seven of them their chi2 would pass 1, with two it passes 5.991 and the reference removes them too; a free landmark with a single edge
  cannot be an outlier at all, it fits any pixel; and a pull at a pose is shared by that pose's edges, which in a window of two or three key-frames
  a step apart are too soft to hold it.  So every constructed outlier is balanced, at its landmark and at its pose:
    - two features of the new key-frame on ONE id displaced by +d and -d: on a new point (it empties and is erased), on a new point with a third,
      exact feature (the front goes, the next observer is in the window), on a tracked point, on a point that returns (it leaves alive again);
    - `sleepers`: twins, two landmarks made side by side and seen by the same key-frames, each with ONE active observation left, which a correction
      event moves sideways by +D and -D.  Their old pixels are then off by r and -r at one place of one key-frame.  A FIXED pair (front observer
      outside the window, src/backend.cpp:175) loses every active observation and leaves alive with its older rows.  A free pair, whose active
      observation is the front, is named by MANY exact features of the new key-frame each, which share the pull; r lies across the epipolar line, where
      no depth takes it away.  If its list goes on with a row of a key-frame that left, this is the case the header of myslam_map_update_batch warns
      about: the front removed, the next observer gone.
  An old observation can only become an outlier by such a move: every observation is exact when it is made, or removed by the optimise that follows."""
import copy

import numpy as np

import backend_ref as br
import map_insert_ref as mi

OK, INVALID = 0, -1
DONE, EMPTY = br.DONE, br.EMPTY
IMG_W, IMG_H = 1241, 376


class _KfRef(int):
    """Feature::mpKF as map_archive_ref reads it (`.kf.id`) and backend_ref reads it (the id itself)"""
    __slots__ = ()

    @property
    def id(self):
        return int(self)


class Obs(br.Obs):
    __slots__ = ()

    def __init__(self, kf, u, v, outlier=False, tag=0):
        super().__init__(kf, u, v, outlier, tag)
        self.kf = _KfRef(kf)


class KeyFrame:
    def __init__(self, kf_id, pose, last_kf, rel_to_last):
        self.id, self.pose, self.last_kf, self.rel_to_last = int(kf_id), np.array(pose, float), last_kf, rel_to_last
        # the two poses mRelativePoseToLastKF was made of, as they stood then
        self.pose_at_insert = self.pose.copy()
        self.last_pose_at_insert = None if last_kf is None else last_kf.pose.copy()


class WholeMap:
    def __init__(self, chain, window, min_dis_th=0.2):
        self.chain, self.window, self.min_dis_th = chain, int(window), float(min_dis_th)
        self.all_kfs, self.active_kfs = {}, {}      # _mumpAllKeyFrames / _mumpActiveKeyFrames: mnKFId -> KeyFrame
        self.all_mps, self.active_mps = {}, {}      # _mumpAllMapPoints / _mumpActiveMapPoints: mnId -> MapPoint (the same objects)
        self.outlier_mps = []                       # _mlistOutlierMapPoints: may name points that are not active, and ids nobody knows
        self.erased = set()                         # every id that was in all_mps and is not any more
        self.cur_kf = None                          # _mpCurrentKF
        self.max_mp_id = -1

    _STATE = ("all_kfs", "active_kfs", "all_mps", "active_mps", "outlier_mps", "erased", "cur_kf", "max_mp_id")

    def clone(self):
        c = WholeMap(self.chain, self.window, self.min_dis_th)
        for k, v in zip(self._STATE, copy.deepcopy(tuple(getattr(self, k) for k in self._STATE))):   # one deepcopy: shared objects stay shared
            setattr(c, k, v)
        return c

    # ------------------------------------------------------------------------------------------------------------------------- views
    def active_map(self):
        """the active part as a backend_ref.Map over the model's own objects (for backend_ref.pack / flatten)"""
        m = br.Map()
        m.kfs = {k: kf.pose for k, kf in self.active_kfs.items()}
        m.mps = dict(self.active_mps)
        m.outlier_list = [i for i in self.outlier_mps if i in self.active_mps]
        return m

    def dist(self, pose_kf, pose_new):
        """(kf.Pose() * Twc).log().norm(), src/map.cpp:87-90"""
        c = self.chain
        return float(c.se3_log_norm(c.mm(c.T_of(np.asarray(pose_kf, float)), c.T_inv(c.T_of(np.asarray(pose_new, float))))))

    def priors_for(self, feats):
        """GetObservations() of every map point a feature names that is alive but not active: the prior rows of the insert, ids ascending"""
        ids = sorted({int(f[0]) for f in feats if f[0] >= 0 and f[0] in self.all_mps and f[0] not in self.active_mps})
        return [(mid, int(o.kf), (o.u, o.v), o.tag, o.outlier) for mid in ids for o in self.all_mps[mid].obs]

    # ------------------------------------------------------------------------------------------------------------------------- calls
    def add_outlier_map_point(self, mid):
        """src/frontend.cpp:263-264: the flag on the object the frontend holds (if it still exists), then Map::AddOutlierMapPoint (src/map.cpp:159-164)"""
        mp = self.all_mps.get(int(mid))
        if mp is not None:
            mp.outlier = True
        self.outlier_mps.append(int(mid))

    def scan(self, new_pose, new_id=None):
        """RemoveOldActiveKeyframe's choice (src/map.cpp:83-107) -> dict(gone, branch, dis: id -> distance, plain: what argmin / argmax would choose)"""
        max_dis, min_dis, max_id, min_id = 0.0, 9999.0, 0, 0                # :83-84
        dis = {}
        for kid in sorted(self.active_kfs):
            if kid == new_id:                                               # :89
                continue
            d = dis[kid] = self.dist(self.active_kfs[kid].pose, new_pose)   # :90
            if d > max_dis:                                                 # :91-93
                max_dis, max_id = d, kid
            elif d < min_dis:                                               # :94-96: never reached by a distance that raised the maximum
                min_dis, min_id = d, kid
        near = min_dis < self.min_dis_th                                    # :103
        lo = min(dis, key=lambda k: dis[k])
        plain = lo if dis[lo] < self.min_dis_th else max(dis, key=lambda k: dis[k])
        return dict(gone=min_id if near else max_id, branch="nearest" if near else "farthest", dis=dis, plain=plain)

    def insert_keyframe(self, ins):
        """The frontend's outlier ids, KeyFrame::CreateKF and Map::InsertKeyFrame for one new key-frame (a map_insert_ref.Insert; its priors are SET here
        from the model's own lists).  -> dict(status, removed_kf_id, branch, quirk, dis, left_alive, returned: [(id, prior rows)], doubled)"""
        rep = dict(status=OK, removed_kf_id=-1, branch=None, quirk=False, dis={}, left_alive=[], returned=[], doubled=0)
        if self.all_kfs and ins.kf_id <= max(self.all_kfs):                 # mnKFId comes from a counter (src/keyframe.cpp:14-15): the device refuses
            rep["status"] = INVALID
            return rep
        ins.priors = self.priors_for(ins.feats)
        for mid in ins.outlier_ids:                                         # src/frontend.cpp:255-270 ran while the frame was tracked
            self.add_outlier_map_point(mid)
        c, last = self.chain, self.cur_kf
        rel = None if last is None else c.p7_of(c.mm(c.T_of(ins.kf_pose), c.T_inv(c.T_of(last.pose))))      # src/frontend.cpp:424-447
        kf = KeyFrame(ins.kf_id, ins.kf_pose, last, rel)
        linked, seen, top = [], {}, self.max_mp_id
        for mid, pos, uv, tag, outlier in ins.feats:                        # src/keyframe.cpp:39-47
            if mid < 0:
                continue
            mp = self.all_mps.get(int(mid))
            if mp is None:                                                  # a point the frontend has just made: Map::InsertMapPoint, src/map.cpp:53-61
                assert mid not in self.erased and mid > top, mid            # mnId comes from a counter (src/mappoint.cpp:7-10)
                mp = self.all_mps[int(mid)] = br.MapPoint(mid, pos)
                self.max_mp_id = max(self.max_mp_id, int(mid))
            elif mid not in self.active_mps and mid not in seen:
                rep["returned"].append((int(mid), len(mp.obs)))
            seen[mid] = seen.get(mid, 0) + 1
            o = Obs(ins.kf_id, uv[0], uv[1], outlier, tag)
            mp.obs.append(o)                                                # AddObservation, src/mappoint.cpp:19-23
            linked.append((mp, o))
        rep["doubled"] = sum(1 for n in seen.values() if n >= 2)
        self.cur_kf = self.all_kfs[kf.id] = self.active_kfs[kf.id] = kf     # src/map.cpp:18-30
        for mp, o in linked:                                                # :35-41
            mp.active_obs.append(o)                                         # AddActiveObservation, src/mappoint.cpp:27-31
            self.active_mps[mp.id] = mp                                     # InsertActiveMapPoint
        if len(self.active_kfs) > self.window:                              # :44-47
            s = self.scan(kf.pose, kf.id)
            gone = s["gone"]
            assert gone in self.active_kfs and gone != kf.id                # .at() (:104, :106)
            rep.update(removed_kf_id=gone, branch=s["branch"], quirk=s["plain"] != gone, dis=s["dis"])
            del self.active_kfs[gone]                                       # :112
            for mp in self.active_mps.values():                             # :113-118: the features of that key-frame that still have their map point
                mp.active_obs = [o for o in mp.active_obs if o.kf != gone]  # RemoveActiveObservation, src/mappoint.cpp:34-43
            rep["left_alive"] = self._remove_old_active_map_points()
        return rep

    def _remove_old_active_map_points(self):
        """src/map.cpp:126-140"""
        out = [mid for mid in sorted(self.active_mps) if not self.active_mps[mid].active_obs]
        for mid in out:
            del self.active_mps[mid]
        return out

    def edges(self):
        """the edges of src/backend.cpp:161-205 in the order of the device's tables: [(MapPoint, Obs)], and the map points that get a vertex with an edge"""
        e, slots = [], []
        for mid in sorted(self.active_mps):
            mp = self.active_mps[mid]
            if mp.outlier:                                                  # :163
                continue
            mine = [(mp, o) for o in mp.active_obs if not o.outlier]        # :183-190
            assert all(o.kf in self.active_kfs for _, o in mine)            # :187
            if mine:
                e += mine; slots.append(mp)
        return e, slots

    def optimize(self, flags, poses, points):
        """Backend::OptimizeActiveMap around its solve.  flags: the tags of the edges whose chi2 passes the threshold (src/backend.cpp:237); poses: mnKFId ->
        the optimised pose of every active key-frame; points: mnId -> the optimised position of the map points that had a vertex.  Both may be callables
        that are only asked when the optimise is not EMPTY.  -> dict(status, mp_report / obs_report by the row BEFORE the call, and what happened)"""
        before = sorted(self.active_mps)
        rows = [(mid, o) for mid in before for o in self.active_mps[mid].obs]
        rep = dict(status=DONE, mp_report=np.zeros(len(before), np.uint8), obs_report=np.zeros(len(rows), np.uint8), front_gone=[], front_in=[],
                   erased_by_ba=[], left_alive=[], listed_erased=[], removed_edges=0)
        edges, slots = self.edges()
        if not edges:                                                       # nothing to optimise: the call returns before anything is removed
            rep["status"] = EMPTY
            rep["listed_waiting"] = [i for i in self.outlier_mps if i in self.all_mps and i not in self.active_mps]
            return rep
        poses = poses() if callable(poses) else poses
        points = points() if callable(points) else points
        row_of = {id(o): r for r, (_, o) in enumerate(rows)}
        front = {mp.id: mp.obs[0] for mp in slots}
        for mp, o in edges:                                                 # :236-251
            if o.tag in flags:
                o.outlier = True
                br._drop(mp.active_obs, o)                                  # RemoveActiveObservation
                br._drop(mp.obs, o)                                         # RemoveObservation, src/mappoint.cpp:46-56
                rep["obs_report"][row_of[id(o)]] = 1; rep["removed_edges"] += 1
                if not mp.obs:                                              # :243-246
                    mp.outlier = True
                    self.outlier_mps.append(mp.id)
                    rep["erased_by_ba"].append(mp.id)
            else:
                o.outlier = False                                           # :249
        for k, kf in self.active_kfs.items():                               # :256-258
            kf.pose = np.array(poses[k], float)
        for mp in slots:                                                    # :259-261: every vertex, also of a point that is about to leave
            mp.pos = np.array(points[mp.id], float)
        for mp in slots:
            if mp.obs and mp.obs[0] is not front[mp.id]:
                (rep["front_in"] if mp.obs[0].kf in self.active_kfs else rep["front_gone"]).append(mp.id)
        for mid in self.outlier_mps:                                        # RemoveAllOutlierMapPoints, src/map.cpp:166-175: the WHOLE list
            if mid in self.all_mps:
                if mid not in self.active_mps:
                    rep["listed_erased"].append(mid)
                del self.all_mps[mid]
                self.erased.add(mid)
            self.active_mps.pop(mid, None)
        self.outlier_mps = []
        rep["left_alive"] = self._remove_old_active_map_points()            # src/map.cpp:126-140
        gone = set()
        for i, mid in enumerate(before):
            if mid not in self.all_mps:
                rep["mp_report"][i] = 2; gone.add(mid)
            elif mid not in self.active_mps:
                rep["mp_report"][i] = 1; gone.add(mid)
        for r, (mid, o) in enumerate(rows):
            if mid in gone and rep["obs_report"][r] == 0:
                rep["obs_report"][r] = 2
        return rep

    def correct(self, rigid=None, moves=None):
        """What a loop correction leaves (src/loopclosing.cpp:612-641 reaches every object): the world moved by the rigid S (pose7; Tcw <- Tcw S^-1,
        p <- S p), then single map points set to new positions"""
        c = self.chain
        if rigid is not None:
            S = c.T_of(np.asarray(rigid, float)); Si = c.T_inv(S)
            for kf in self.all_kfs.values():
                kf.pose = c.p7_of(c.mm(c.T_of(kf.pose), Si))
            for mp in self.all_mps.values():
                mp.pos = c.mv(S[:3, :3], mp.pos) + S[:3, 3]
        for mid, p in (moves or {}).items():
            self.all_mps[mid].pos = np.array(p, float)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# histories

class Event:
    """kind: "correct" (rigid, moves) | "insert" (ins) | "refused" (ins: an id that is not above the last) | "capacity" (ins: one key-frame more than the
    archive's caps hold) | "optimize" (flags: the tags of the constructed outlier edges).  meta: what the generator aimed at."""

    def __init__(self, kind, ins=None, flags=frozenset(), rigid=None, moves=None, meta=None):
        self.kind, self.ins, self.flags, self.rigid, self.moves, self.meta = kind, ins, frozenset(flags), rigid, moves, dict(meta or {})


MARGIN = 0.01          # what the issue asks of the removal branch
AIM = 0.015            # what a candidate pose must have, so that the device's numbers (equal to the oracle's to ~1e-9) choose the same candidate
ANCHORS = 10           # edges of fixed landmarks in every key-frame of the window before an old observation is made an outlier
MANY = 12              # features of the new key-frame on a free sleeper
OUT_PX = 60.0          # a gross outlier's least displacement


def _unit(v):
    return v / np.sqrt(float(np.dot(v, v)))


def _rotvec_q(w):
    a = np.sqrt(float(np.dot(w, w)))
    if a < 1e-12:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(a / 2) * w / a, [np.cos(a / 2)]])


def _pose_at(chain, center, w):
    """Tcw (qx qy qz qw tx ty tz) of a camera at `center` with the rotation vector w (of Rcw)"""
    q = _rotvec_q(np.asarray(w, float))
    R = chain.q_to_R(q)
    return np.concatenate([q, -chain.mv(R, np.asarray(center, float))])


def _center(chain, pose):
    R = chain.q_to_R(np.asarray(pose[:4], float))
    return -chain.mv(R.T, np.asarray(pose[4:], float))


def project(chain, K, pose, p):
    """-> (pixel, depth) of the world point p in the camera `pose`"""
    R = chain.q_to_R(np.asarray(pose[:4], float))
    pc = chain.mv(R, np.asarray(p, float)) + np.asarray(pose[4:], float)
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]]), float(pc[2])


def margins_ok(s, th, margin):
    """every comparison the scan made, and the one with the threshold, is decided by at least `margin`"""
    d = sorted(s["dis"].values())
    return all(b - a >= margin for a, b in zip(d, d[1:])) and all(abs(x - th) >= margin for x in d) and d[0] >= margin


def _plan_pose(rng, m, mode):
    """the new key-frame's pose: `mode` in free (nothing leaves) | nearest | farthest | quirk.  Twelve candidates are drawn whatever happens (the stream of
    random numbers must not depend on the model's numbers); the first whose scan does what `mode` says with AIM to spare is taken.
    -> (pose, scan or None, the mode that was met)"""
    chain = m.chain
    ids = sorted(m.active_kfs)
    last = m.cur_kf
    draws = [(rng.uniform(-1, 1, 3), rng.uniform(0.06, 0.14), rng.uniform(0.3, 0.6), rng.uniform(-0.02, 0.02, 3), int(rng.integers(1 << 30))) for _ in range(12)]
    if last is None:
        return _pose_at(chain, np.zeros(3), draws[0][3]), None, "free"
    c_last = _center(chain, last.pose)
    fwd = lambda dr, k=1.0: c_last + np.array([0.25 * dr[0][0], 0.1 * dr[0][1], k * dr[2]])
    if mode == "free":
        return _pose_at(chain, fwd(draws[0]), draws[0][3]), None, "free"
    for want in (mode, "farthest", "far2"):
        for dr in draws:
            if want == "nearest":
                v = ids[1 + dr[4] % (len(ids) - 1)] if len(ids) > 1 else ids[0]
                pose = _pose_at(chain, _center(chain, m.active_kfs[v].pose) + dr[1] * _unit(dr[0]), dr[3])
            elif want == "quirk":
                v = ids[0]
                pose = _pose_at(chain, _center(chain, m.active_kfs[v].pose) + dr[1] * _unit(dr[0]), dr[3])
            else:
                pose = _pose_at(chain, fwd(dr, 1.0 if want == "farthest" else 2.0), dr[3])
            s = m.scan(pose)
            if not margins_ok(s, m.min_dis_th, AIM):
                continue
            met = "quirk" if s["plain"] != s["gone"] else s["branch"]
            if met == ("farthest" if want == "far2" else want) and (want != "nearest" or s["gone"] == v):
                return pose, s, met
    raise AssertionError("no candidate pose meets the margins")


def history(seed, m, K, n_kf, n_steps=None, extras=(), first_points=30, max_active=48, kf_id0=3, mp_id0=100):
    """Events of one history on the WholeMap `m` (empty at the start; the consumer applies every event to `m` before it asks for the next one).
    n_kf key-frames, then refused inserts and optimises without a flag up to n_steps steps (an item that has finished, next to running ones).
    extras: "refused" (a refused insert in the middle), "empty" (the frontend lists every active point and some that are not active; the key-frame links
    no point; the optimise is EMPTY), "rigid" (a correction moves the whole world), "capacity" (one key-frame more at the end)."""
    chain = m.chain
    rng = np.random.default_rng([int(seed), 0x3A9])
    n_steps = n_steps or n_kf
    next_kf, next_mp, tag = [kf_id0], [mp_id0], [0]
    twin, m_pos = {}, {}
    k_refused = n_kf // 2 if "refused" in extras else -1
    k_empty = (2 * n_kf) // 3 if "empty" in extras else -1
    k_rigid = n_kf // 3 + 1 if "rigid" in extras else -1
    W = m.window

    def new_tag():
        tag[0] += 1
        return tag[0]

    def visible(pose, p):
        uv, z = project(chain, K, pose, p)
        return z > 4.0 and -300 < uv[0] < IMG_W + 300 and -300 < uv[1] < IMG_H + 300

    def feat(mid, pose, p, shift=(0.0, 0.0)):
        uv, _ = project(chain, K, pose, p)
        t = new_tag()
        return (int(mid), tuple(np.asarray(p, float)), (np.float32(uv[0] + shift[0]), np.float32(uv[1] + shift[1])), t, False), t

    k, refused_done = -1, False
    for _ in range(n_steps):                                                # every step is an insert call and an optimise, whatever they do
        k += 1
        if k >= n_kf:                                                       # finished: the item only sees refused inserts and idle optimises
            last = m.cur_kf
            yield Event("refused", ins=mi.Insert(last.id - int(rng.integers(0, 2)), last.pose, [(-1, (0.0, 0.0, 0.0), (1.0, 2.0), new_tag(), False)]))
            yield Event("optimize", meta=dict(idle=True))
            continue
        if k == k_refused and not refused_done:                             # a step of its own: the optimise that follows finds the window as it was
            last = m.cur_kf
            fs = [feat(mid, last.pose, m.active_mps[mid].pos)[0] for mid in sorted(m.active_mps)[:5]] + [(next_mp[0] + 50, (0.0, 0.0, 9.0), (3.0, 4.0), new_tag(), False)]
            yield Event("refused", ins=mi.Insert(last.id, last.pose, fs, outlier_ids=sorted(m.active_mps)[:2]))
            yield Event("optimize", meta=dict(idle=True))
            k, refused_done = k - 1, True
            continue
        if k == k_rigid:
            yield Event("correct", rigid=np.concatenate([_rotvec_q(rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.5, 0.5, 3)]))
        # ---- the pose: which branch of src/map.cpp:103-107 the insert takes
        u = rng.random()
        mode = "free" if len(m.active_kfs) < W else ("nearest" if u < 0.4 else ("farthest" if u < 0.7 else "quirk"))
        pose, s, met = _plan_pose(rng, m, mode)
        victim = s["gone"] if s else None
        stay = set(m.active_kfs) - {victim}
        kf_id = next_kf[0] + int(rng.integers(0, 3)); next_kf[0] = kf_id + 1
        # ---- the pools, from structure alone (visibility is a number, but it only decides between a feature and none on a margin of hundreds of pixels)
        ok = [mid for mid in sorted(m.active_mps) if not m.active_mps[mid].outlier and visible(pose, m.active_mps[mid].pos)]
        away = [mid for mid in sorted(m.all_mps) if mid not in m.active_mps and not m.all_mps[mid].outlier]
        eff = {mid: [o for o in m.active_mps[mid].active_obs if o.kf in stay] for mid in ok}
        fixed = {mid: m.active_mps[mid].obs[0].kf not in stay for mid in ok}
        perm = lambda xs: [xs[i] for i in rng.permutation(len(xs))] if xs else []
        feats, flags, moves, groups, meta = [], set(), {}, [], dict(mode=met, aimed=[])
        outlier_ids = []
        if k == k_empty:
            outlier_ids = sorted(m.active_mps) + perm(away)[:5]
            feats = [(-1, (0.0, 0.0, 0.0), (float(i), 2.0), new_tag(), False) for i in range(3)]
            meta["empty"] = True
        else:
            # eff: the active observations the insert will leave.  A sleeper has ONE of them.  free "gone": it is the front and the list goes on
            # (with a row of a key-frame that left); free "in": it is the only row; "fixed": the front observer is outside the window
            one = [mid for mid in ok if len(eff[mid]) == 1]
            kind_of = {mid: ("fixed" if fixed[mid] else ("gone" if len(m.active_mps[mid].obs) >= 2 else "in")) for mid in one
                       if fixed[mid] or eff[mid][0] is m.active_mps[mid].obs[0]}

            def twin_pairs(want_fixed):
                """twins (two landmarks made side by side and seen by the same key-frames) that are both sleepers on one key-frame, "gone" ones first"""
                out = [(p, twin[p]) for p in sorted(kind_of) if p in twin and p < twin[p] and twin[p] in kind_of and kind_of[p] == kind_of[twin[p]]
                       and (kind_of[p] == "fixed") == want_fixed and eff[p][0].kf == eff[twin[p]][0].kf]
                return sorted(perm(out), key=lambda pq: kind_of[pq[0]] != "gone")

            # every group: (kind, ids); the order is the priority under the 10 % cap
            groups += [("sleepers", pq) for pq in twin_pairs(False)[:1]]
            groups += [("fixed_sleepers", pq) for pq in twin_pairs(True)[:1]]
            taken = {i for g in groups for i in g[1]}
            rest = [mid for mid in ok if mid not in taken]
            coin = {}
            for mid in rest:                                                # twins are seen together, and only now and then: many have one active row
                key = min(mid, twin.get(mid, mid))
                if key not in coin:
                    coin[key] = rng.random() < (0.45 if mid in twin else 0.8)
            tracked = [mid for mid in rest if coin[min(mid, twin.get(mid, mid))]]
            back = perm([mid for mid in away if visible(pose, m.all_mps[mid].pos)])
            back = sorted(back, key=lambda i: -min(len(m.all_mps[i].obs), 2))[:3] if rng.random() < 0.8 else []
            n_new = first_points if not m.all_kfs else int(rng.integers(5, 10))
            n_new = max(0, min(n_new, max_active - 4 - len(m.active_mps) - len(back)))
            if len(ok) < 5:                                                 # after a wipe: the key-frame needs points of its own
                n_new = max(n_new, min(12, max_active - len(m.active_mps) - len(back)))
            pair_new = rng.random() < 0.6 and n_new >= 3
            triple_new = rng.random() < 0.6 and n_new >= 3
            pair_old = rng.random() < 0.3
            pair_back = rng.random() < 0.5 and len(back) >= 1
            double_exact = rng.random() < 0.5
            # the frontend's outlier ids: an active point this key-frame does not name, points that are not active, an id nobody knows, an erased id
            single = [mid for mid in tracked if mid not in twin]
            if single and rng.random() < 0.25:
                outlier_ids.append(single[int(rng.integers(len(single)))])
                tracked.remove(outlier_ids[-1])
            quiet = [mid for mid in away if mid not in back]
            if quiet and rng.random() < 0.6:
                outlier_ids += perm(quiet)[:1 + int(rng.random() < 0.3)]
            if rng.random() < 0.3:
                outlier_ids.append(10 ** 7 + k)
            if m.erased and rng.random() < 0.2:
                outlier_ids.append(sorted(m.erased)[int(rng.integers(len(m.erased)))])
            if pair_back:
                groups.append(("pair_back", (back[0],)))
            if triple_new:
                groups.append(("triple_new", ()))
            if pair_old and single:
                groups.append(("pair_old", (single[0],)))
            if pair_new:
                groups.append(("pair_new", ()))
            shifts = {g: _unit(rng.normal(size=2)) * rng.uniform(OUT_PX + 10, OUT_PX + 40) for g in groups}
            extra_exact = rng.random() < 0.5
            # ---- the 10 % cap: the edges of the window as the insert will leave it
            n_edges = sum(len(eff[mid]) for mid in ok if mid not in outlier_ids) + len(tracked) + len(back) + n_new + len(groups)
            cost = dict(sleepers=2, fixed_sleepers=2, pair_back=2, triple_new=2, pair_old=2, pair_new=2)
            # twins balance one another up to the little their places differ; in a window without fixed landmarks (two poses a step apart, landmarks
            # seen twice) even that little moves everything, so old observations are only touched in a window that fixed landmarks hold in place
            anchors = min([sum(1 for mid in tracked if fixed[mid])] + [sum(1 for mid in rest if fixed[mid] for o in eff[mid] if o.kf == kid) for kid in stay])
            kept, spent = [], 0
            for g in groups:
                if spent + cost[g[0]] <= 0.1 * n_edges and (anchors >= ANCHORS or g[0] not in ("sleepers", "fixed_sleepers")):
                    kept.append(g); spent += cost[g[0]]
            dropped = [i for g in groups if g not in kept and g[0] in ("sleepers", "fixed_sleepers") for i in g[1]]
            tracked = sorted(tracked + dropped)
            for kind, ids in kept:
                d = shifts[(kind, ids)]
                meta["aimed"].append(kind)
                if kind in ("sleepers", "fixed_sleepers"):
                    for sgn, mid in zip((1.0, -1.0), ids):                  # opposite residuals at one pixel and one depth: no pull at any pose
                        mp, a = m.active_mps[mid], eff[mid][0]
                        pa = m.active_kfs[a.kf].pose
                        u0, za = project(chain, K, pa, mp.pos)
                        side = lambda dv: mp.pos + chain.mv(chain.q_to_R(pa[:4]).T, np.array([sgn * dv[0] * za / K[0], sgn * dv[1] * za / K[1], 0.0]))
                        p2 = side(d)
                        if kind == "sleepers":                              # a free landmark would follow a pull along the epipolar line in depth: the
                            for _ in range(6):                              # residual is laid across that line as it runs where the landmark ends up
                                v0, _ = project(chain, K, pa, p2)
                                v1, _ = project(chain, K, pa, p2 + 0.2 * (p2 - _center(chain, pose)))
                                e = _unit(v1 - v0)
                                p2 = side(np.array([-e[1], e[0]]) * np.sqrt(float(np.dot(d, d))))
                            meta["aimed"].append("front_next_" + kind_of[mid])
                        moves[mid] = p2
                        r = project(chain, K, pa, p2)[0] - np.array([a.u, a.v], float)
                        assert np.linalg.norm(r) >= OUT_PX, (mid, r)
                        flags.add(a.tag)
                        if kind == "sleepers":                              # the inliers that share the outlier's pull: chi2 (5.991 / MANY)^2 each
                            feats += [feat(mid, pose, p2)[0] for _ in range(MANY)]
                elif kind in ("pair_old", "pair_back"):                     # two features of the new key-frame on one id, displaced by +d and -d
                    src = m.all_mps[ids[0]]
                    for sgn in (1.0, -1.0):
                        f, t = feat(ids[0], pose, src.pos, shift=sgn * d); feats.append(f); flags.add(t)
                    tracked = [i for i in tracked if i != ids[0]]
                    back = [i for i in back if i != ids[0]]
            for n, mid in enumerate(tracked):
                feats.append(feat(mid, pose, m.active_mps[mid].pos)[0])
                if double_exact and n == 0:
                    feats.append(feat(mid, pose, m.active_mps[mid].pos)[0])
                if n % 11 == 5:
                    feats.append((-1, (0.0, 0.0, 0.0), (float(n), 7.0), new_tag(), False))
            for mid in back:
                feats.append(feat(mid, pose, m.all_mps[mid].pos)[0])
            R = chain.q_to_R(pose[:4])
            made = []
            for n in range(n_new):
                z = rng.uniform(12.0, 35.0)
                px = np.array([rng.uniform(40, IMG_W - 40), rng.uniform(20, IMG_H - 20)])
                pw = chain.mv(R.T, np.array([(px[0] - K[2]) * z / K[0], (px[1] - K[3]) * z / K[1], z]) - pose[4:])
                mid = next_mp[0] + int(rng.integers(0, 3)); next_mp[0] = mid + 1
                if n in (4, 6) and made:                                    # a twin: beside the landmark made before it
                    pw = m_pos[made[-1]] + chain.mv(R.T, np.array([0.03, 0.02, 0.0]))
                    twin[mid] = made[-1]; twin[made[-1]] = mid
                m_pos[mid] = pw
                made.append(mid)
                if n == 0 and ("pair_new", ()) in kept:
                    for sgn in (1.0, -1.0):
                        f, t = feat(mid, pose, pw, shift=sgn * shifts[("pair_new", ())]); feats.append(f); flags.add(t)
                elif n == 1 and ("triple_new", ()) in kept:                 # in feature order +d, -d, exact: the front goes, the next observer is this key-frame
                    triple = []
                    for sgn in (1.0, -1.0):
                        f, t = feat(mid, pose, pw, shift=sgn * shifts[("triple_new", ())]); triple.append(f); flags.add(t)
                    triple.append(feat(mid, pose, pw)[0])
                else:
                    feats.append(feat(mid, pose, pw)[0])
            feats = [feats[i] for i in rng.permutation(len(feats))]       # mvpFeaturesLeft is in no order of ids
            if ("triple_new", ()) in kept:
                at = sorted(int(i) for i in rng.integers(0, len(feats) + 1, 3))
                for i, f in zip(at[::-1], triple[::-1]):
                    feats.insert(i, f)
            meta.update(n_edges=n_edges, n_out=len(flags))
        if moves:
            yield Event("correct", moves=moves)
        yield Event("insert", ins=mi.Insert(kf_id, pose, feats, outlier_ids=outlier_ids), meta=meta)
        yield Event("optimize", flags=flags, meta=meta)
    if "capacity" in extras:
        pose, s, met = _plan_pose(rng, m, "farthest" if len(m.active_kfs) >= W else "free")
        R = chain.q_to_R(pose[:4])
        pw = chain.mv(R.T, np.array([0.5, 0.2, 20.0]) - pose[4:])
        fs = [feat(mid, pose, m.active_mps[mid].pos)[0] for mid in sorted(m.active_mps)[:8]] + [feat(next_mp[0] + 1, pose, pw)[0]]
        yield Event("capacity", ins=mi.Insert(next_kf[0] + 1, pose, fs))
