"""Map::InsertKeyFrame (reference src/map.cpp:17-48 with KeyFrame::CreateKF's observation loop, src/keyframe.cpp:34-50, RemoveOldActiveKeyframe :78-120,
RemoveOldActiveMapPoints :126-140, AddOutlierMapPoint :159-164, src/mappoint.cpp:19-44) as a literal walk over backend_ref's containers, with the
distance passed in as a function; and a packer for the new key-frame's inputs of myslam_backend_insert_keyframe_batch.  Test helper, no GPU."""
import numpy as np

import backend_ref as br

OK, INVALID, CAPACITY = 0, -1, -3              # MYSLAM_OK, MYSLAM_ERR_INVALID, MYSLAM_ERR_CAPACITY


class Insert:
    """One new key-frame.  feats: [(mp id or -1, (x, y, z), (u, v), tag, outlier)] in mvpFeaturesLeft order; priors: [(mp id, kf id, (u, v), tag, outlier)]
    = GetObservations() of map points that are not in the active set, ids non-decreasing; outlier_ids: what Map::AddOutlierMapPoint was given."""

    def __init__(self, kf_id, kf_pose, feats=(), priors=(), outlier_ids=()):
        self.kf_id, self.kf_pose = int(kf_id), np.array(kf_pose, float)
        self.feats, self.priors, self.outlier_ids = list(feats), list(priors), list(outlier_ids)


def insert_walk(m, ins, window, min_dis_th, dist, caps=None):
    """Map::InsertKeyFrame on `m` (changed in place unless refused).  dist(pose7 of a key-frame, pose7 of the new one, the key-frame's INPUT row) ->
    |log(T_kf T_new^-1)|.  caps = (kf_cap, mp_cap, obs_cap) or None.  Returns the reports of myslam_backend_insert_keyframe_batch by INPUT row."""
    kf_in, mp_in = sorted(m.kfs), sorted(m.mps)
    rep = dict(status=OK, feat_row=np.full(len(ins.feats), -1, np.int32), mp_new_row=np.full(len(mp_in), -1, np.int32), removed_kf_id=-1,
               removed_kf_row=-1, dis=np.full(len(kf_in), -1.0), branch=None)

    def refused(code):
        rep["status"] = code
        return rep

    if window < 1 or (kf_in and ins.kf_id <= kf_in[-1]):                    # mnKFId comes from a counter
        return refused(INVALID)
    if any(f[0] < -1 for f in ins.feats) or any(a[0] > b[0] for a, b in zip(ins.priors, ins.priors[1:])):
        return refused(INVALID)
    if any(o.kf not in m.kfs for mp in m.mps.values() for o in mp.active_obs):
        return refused(INVALID)
    w = m.clone()                                                           # everything is decided before anything is written
    for mid in ins.outlier_ids:                                             # map.cpp:159-164 + frontend.cpp:263: ids outside the table are ignored
        if mid in w.mps:
            w.mps[mid].outlier = True
            if mid not in w.outlier_list:
                w.outlier_list.append(mid)
    w.kfs[ins.kf_id] = ins.kf_pose.copy()                                   # map.cpp:24-30
    feat_obs = []
    for mid, pos, uv, tag, outlier in ins.feats:                            # keyframe.cpp:41-47 (AddObservation) + map.cpp:35-41
        if mid == -1:                                                       # mpMapPoint.lock() == nullptr
            feat_obs.append(None)
            continue
        mp = w.mps.get(mid)
        if mp is None:                                                      # InsertActiveMapPoint: the point comes with the observations it has
            mp = br.MapPoint(mid, pos)
            mp.obs = [br.Obs(k, puv[0], puv[1], po, ptag) for pid, k, puv, ptag, po in ins.priors if pid == mid]
            w.mps[mid] = mp
        o = br.Obs(ins.kf_id, uv[0], uv[1], outlier, tag)
        mp.obs.append(o); mp.active_obs.append(o)                           # both push_back
        feat_obs.append(o)
    if caps is not None and (len(w.kfs) > caps[0] or len(w.mps) > caps[1] or len(br.rows_of(w)) > caps[2]):
        return refused(CAPACITY)
    if len(w.kfs) > window:                                                 # map.cpp:44
        max_dis, min_dis, max_id, min_id = 0.0, 9999.0, 0, 0                # map.cpp:83-98
        for row, kid in enumerate(kf_in):
            dis = float(dist(w.kfs[kid], ins.kf_pose, row))
            rep["dis"][row] = dis
            if dis > max_dis:
                max_dis, max_id = dis, kid
            elif dis < min_dis:
                min_dis, min_id = dis, kid
        rep["branch"] = "nearest" if min_dis < min_dis_th else "farthest"
        gone = min_id if min_dis < min_dis_th else max_id                   # :103-107
        if gone not in kf_in:                                               # .at() throws
            rep["dis"][:] = -1.0
            rep["branch"] = None
            return refused(INVALID)
        rep["removed_kf_id"], rep["removed_kf_row"] = gone, kf_in.index(gone)
        del w.kfs[gone]                                                     # :112
        for mp in w.mps.values():                                           # :113-118 RemoveActiveObservation; the row stays in GetObservations()
            mp.active_obs = [o for o in mp.active_obs if o.kf != gone]
        for mid in [k for k, mp in w.mps.items() if not mp.active_obs]:     # :126-140
            del w.mps[mid]
    row_of = {id(o): r for r, (_, _, o) in enumerate(br.rows_of(w))}
    for f, o in enumerate(feat_obs):
        if o is not None:
            rep["feat_row"][f] = row_of[id(o)]
    after = {mid: i for i, mid in enumerate(sorted(w.mps))}
    for i, mid in enumerate(mp_in):
        rep["mp_new_row"][i] = after.get(mid, -1)
    m.kfs, m.mps, m.outlier_list = w.kfs, w.mps, w.outlier_list
    return rep


INPUTS = ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags", "n_feat", "prior_mp_id", "prior_kf_id", "prior_uv",
          "prior_tag", "prior_flags", "n_prior", "outlier_mp_id", "n_outlier")
_FILL = dict(feat_mp_id=-66, feat_mp_pos=-6.5, feat_uv=-5.5, feat_tag=-65, feat_flags=0xAA, prior_mp_id=-64, prior_kf_id=-63, prior_uv=-4.5,
             prior_tag=-62, prior_flags=0xAB, outlier_mp_id=-61)


def pack_inputs(inss, feat_cap, prior_cap, outlier_cap):
    """The new key-frames of a batch as the strided arrays of myslam_backend_insert_keyframe_batch (numpy); slots from a count on hold a sentinel"""
    B = len(inss)
    out = dict(new_kf_id=np.array([i.kf_id for i in inss], np.int64), new_kf_pose=np.array([i.kf_pose for i in inss], np.float64).reshape(B, 7),
               feat_mp_id=np.full((B, feat_cap), _FILL["feat_mp_id"], np.int64), feat_mp_pos=np.full((B, feat_cap, 3), _FILL["feat_mp_pos"], np.float64),
               feat_uv=np.full((B, feat_cap, 2), _FILL["feat_uv"], np.float32), feat_tag=np.full((B, feat_cap), _FILL["feat_tag"], np.int32),
               feat_flags=np.full((B, feat_cap), _FILL["feat_flags"], np.uint8), n_feat=np.array([len(i.feats) for i in inss], np.int32),
               prior_mp_id=np.full((B, prior_cap), _FILL["prior_mp_id"], np.int64), prior_kf_id=np.full((B, prior_cap), _FILL["prior_kf_id"], np.int64),
               prior_uv=np.full((B, prior_cap, 2), _FILL["prior_uv"], np.float32), prior_tag=np.full((B, prior_cap), _FILL["prior_tag"], np.int32),
               prior_flags=np.full((B, prior_cap), _FILL["prior_flags"], np.uint8), n_prior=np.array([len(i.priors) for i in inss], np.int32),
               outlier_mp_id=np.full((B, outlier_cap), _FILL["outlier_mp_id"], np.int64), n_outlier=np.array([len(i.outlier_ids) for i in inss], np.int32))
    for b, i in enumerate(inss):
        assert len(i.feats) <= feat_cap and len(i.priors) <= prior_cap and len(i.outlier_ids) <= outlier_cap
        for f, (mid, pos, uv, tag, outlier) in enumerate(i.feats):
            out["feat_mp_id"][b, f] = mid; out["feat_mp_pos"][b, f] = pos; out["feat_uv"][b, f] = uv; out["feat_tag"][b, f] = tag
            out["feat_flags"][b, f] = br.OUTLIER if outlier else 0
        for p, (mid, kid, uv, tag, outlier) in enumerate(i.priors):
            out["prior_mp_id"][b, p] = mid; out["prior_kf_id"][b, p] = kid; out["prior_uv"][b, p] = uv; out["prior_tag"][b, p] = tag
            out["prior_flags"][b, p] = br.OUTLIER if outlier else 0
        out["outlier_mp_id"][b, :len(i.outlier_ids)] = i.outlier_ids
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# hand-made inputs

IDENT = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def shifted(x, y=0.0, z=0.0):
    """Tcw of a pure translation: with exact binary fractions the distances between such poses are exact"""
    return np.array([0, 0, 0, 1, x, y, z], float)


def small_map(kf_ids, kf_poses, n_mp, rows_per_mp=2, first_mp_id=100, mp_step=3, seed=0, tag0=1):
    """A map of len(kf_ids) key-frames and n_mp map points with ids first_mp_id, + mp_step, ...; map point j has `rows_per_mp` ACTIVE rows on the
    key-frames j, j + 1, ... (mod) and, every fourth point, a leading row of a key-frame that left the window"""
    rng = np.random.default_rng([seed, 0x1415])
    m = br.Map()
    for k, p in zip(kf_ids, kf_poses):
        m.kfs[int(k)] = np.array(p, float)
    tag = tag0
    for j in range(n_mp):
        mp = br.MapPoint(first_mp_id + mp_step * j, rng.uniform(-4, 4, 3) + (0, 0, 12))
        if j % 4 == 3:
            mp.obs.append(br.Obs(-5 - (j % 3), *rng.uniform(10, 600, 2), False, tag)); tag += 1
        for n in range(rows_per_mp if kf_ids else 0):
            o = br.Obs(kf_ids[(j + n) % len(kf_ids)], *rng.uniform(10, 600, 2), rng.random() < 0.1, tag); tag += 1
            mp.obs.append(o); mp.active_obs.append(o)
        m.mps[mp.id] = mp
    return m


def feats_on(ids, seed=0, tag0=5000, outlier_every=7):
    """one feature per entry of `ids` (-1 = no map point), with positions, pixels and tags that differ from feature to feature"""
    rng = np.random.default_rng([seed, 0x2718])
    return [(int(i), tuple(rng.uniform(-4, 4, 3) + (0, 0, 12)), tuple(np.float32(rng.uniform(10, 600, 2))), tag0 + f, i >= 0 and f % outlier_every == 3)
            for f, i in enumerate(ids)]


def rand_pose(rng, max_angle=0.9, max_t=1.0):
    """Tcw with a rotation below max_angle (two of them differ by less than 2 rad) and a translation within max_t"""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = rng.uniform(0.05, max_angle)
    return np.concatenate([ax * np.sin(a / 2), [np.cos(a / 2)], rng.uniform(-max_t, max_t, 3)])


def sized_case(n_mp, n_obs, n_feat, seed, n_kf=4):
    """A map of n_kf key-frames at the window's limit with exactly n_mp map points and n_obs rows (row r belongs to map point r % n_mp: ACTIVE rows of
    the key-frames in turn, every fifth a row of a key-frame that left), and a key-frame of n_feat features: table ids, new ids between and above
    them, every sixth none"""
    rng = np.random.default_rng([seed, 0x5151])
    kf_ids = [2 + 3 * i for i in range(n_kf)]
    m = br.Map()
    for k in kf_ids:
        m.kfs[k] = rand_pose(rng)
    for j in range(n_mp):
        m.mps[10 + 2 * j] = br.MapPoint(10 + 2 * j, rng.uniform(-4, 4, 3) + (0, 0, 12))
    for r in range(n_obs):
        mp = m.mps[10 + 2 * (r % n_mp)]
        if r % 5 == 4:
            mp.obs.append(br.Obs(-9, *rng.uniform(10, 600, 2), False, 100000 + r))
        else:
            o = br.Obs(kf_ids[(r // n_mp + r) % n_kf], *rng.uniform(10, 600, 2), r % 11 == 0, 100000 + r)
            mp.obs.append(o); mp.active_obs.append(o)
    pool = [10 + 2 * j for j in range(n_mp)] + [11 + 2 * j for j in range(0, n_mp, 3)] + [10 + 2 * n_mp + 5 + j for j in range(4)]
    ids = [(-1 if f % 6 == 5 else int(pool[rng.integers(len(pool))])) for f in range(n_feat)]
    ins = Insert(kf_ids[-1] + 2, rand_pose(rng), feats_on(ids, seed))
    return dict(m=m, ins=ins, window=n_kf, th=0.2)


def _base(kf_poses=None, n_mp=6, kf_ids=(3, 5, 8)):
    kf_poses = kf_poses or [shifted(4.0 * (i + 1)) for i in range(len(kf_ids))]
    return small_map(list(kf_ids), kf_poses, n_mp)


def cases():
    """name -> dict(m, ins, window, th[, victim_row][, exact = the distances by row][, gaps][, status])"""
    c = {}
    big = 10                                                                # a window that is not exceeded
    for name, ids in (("new_below", [50, 51]), ("new_between", [101, 104]), ("new_above", [200, 201]),
                      ("interleaved", [200, 101, 103, 50, 104, 106, -1, 116, 100]), ("all_on_one_table_id", [106] * 5), ("all_on_one_new_id", [107] * 5),
                      ("two_and_three_on_one_id", [103, 103, 107, 107, 107, 109, 109, 109, 120, 120]), ("all_without_map_point", [-1] * 4)):
        c[name] = dict(m=_base(), ins=Insert(9, shifted(0.5), feats_on(ids)), window=big, th=0.2)
        c[name + "_removal"] = dict(m=_base(), ins=Insert(9, shifted(0.5), feats_on(ids)), window=3, th=0.2)
    m = _base(); m.mps[106].outlier = True; m.outlier_list.append(106)
    c["feature_on_outlier_map_point"] = dict(m=m, ins=Insert(9, shifted(0.5), feats_on([106, 103])), window=big, th=0.2)
    # prior rows: 104 is new (its key-frames: 5 in the window, 77 outside, 3 the victim: the nearest below the threshold after a farther one),
    # 103 is in the table, 105 is named by no feature
    poses = [shifted(0.125), shifted(2.0), shifted(3.0)]
    pri = [(103, 5, (1.5, 2.5), 901, False), (104, 5, (3.5, 4.5), 902, True), (104, 77, (5.5, 6.5), 903, False), (104, 3, (7.5, 8.5), 904, False),
           (105, 5, (9.5, 10.5), 905, False)]
    c["prior_rows"] = dict(m=_base(poses), ins=Insert(9, shifted(0.0), feats_on([104, 103, 104, 200]), pri), window=big, th=0.2)
    poses = [shifted(2.0), shifted(3.0), shifted(0.125)]                   # the scan: 2.0 max, 3.0 max, 0.125 min -> key-frame 8 leaves
    pri = [(p[0], {3: 8, 5: 5}.get(p[1], p[1])) + p[2:] for p in pri]
    c["prior_rows_removal"] = dict(m=_base(poses), ins=Insert(9, shifted(0.0), feats_on([104, 103, 104, 200]), pri), window=3, th=0.2, victim_row=2)
    c["outlier_ids"] = dict(m=_base(), ins=Insert(9, shifted(0.5), feats_on([103, 200]), outlier_ids=[103, 999, 112]), window=big, th=0.2)
    c["outlier_ids_removal"] = dict(m=_base(), ins=Insert(9, shifted(0.5), feats_on([103, 200]), outlier_ids=[103, 999, 112]), window=3, th=0.2)
    m = _base(); lone = br.MapPoint(104, (1.0, 2.0, 9.0)); lone.obs.append(br.Obs(3, 11.0, 12.0, False, 77)); m.mps[104] = lone
    c["window_not_exceeded"] = dict(m=m, ins=Insert(9, shifted(0.5), feats_on([103, 300])), window=4, th=0.2)
    # the victim's place: rotations, distances with gaps; rows of every key-frame in the table
    rng = np.random.default_rng(0xF00D)
    far = [np.concatenate([rand_pose(rng)[:4], t]) for t in ((6.0, 0, 0), (0, 7.0, 0), (0, 0, 8.0), (5.0, 5.0, 0))]
    q = rand_pose(rng)[:4]                                                  # one rotation for all: the distances are 10, 1, 2, 1.5 -> the first is the farthest
    same = [np.concatenate([q, t]) for t in ((10.0, 0, 0), (1.0, 0, 0), (0, 2.0, 0), (0, 0, 1.5))]
    for name, old, new, row in (("victim_first", same, np.concatenate([q, (0.0, 0.0, 0.0)]), 0),
                                ("victim_middle", far, far[2] + np.array([0, 0, 0, 0, 0.03, 0.02, 0.01]), 2),
                                ("victim_last", far, far[3] + np.array([0, 0, 0, 0, 0.02, 0.03, 0.01]), 3)):
        c[name] = dict(m=small_map([3, 5, 8, 9], old, 9, rows_per_mp=2), ins=Insert(12, new, feats_on([100, 103, 106, 130, 131, -1])), window=4, th=0.2,
                       victim_row=row, gaps=True)
    # the rule's corners: pure translations, exact distances
    for name, ds, th, row in (("ascending", [0.0625, 0.125, 0.5], 0.2, 2), ("descending", [0.5, 0.125, 0.0625], 0.2, 2), ("on_the_threshold", [0.5, 0.25], 0.25, 0),
                              ("equal_maxima", [0.5, 0.5, 0.125, 0.125], 0.0625, 0), ("equal_minima", [0.5, 0.5, 0.125, 0.125], 0.2, 2),
                              ("all_zero", [0.0, 0.0, 0.0], 0.2, 0), ("one_other", [0.75], 0.2, 0)):
        ids = [2 + 2 * i for i in range(len(ds))]
        c[name] = dict(m=small_map(ids, [shifted(1.0 + d) for d in ds], 7), ins=Insert(20, shifted(1.0), feats_on([100, 103, 150])), window=len(ds), th=th,
                       victim_row=row, exact=ds)
    nan = np.full(7, np.nan)
    c["all_nan_with_key_frame_0"] = dict(m=small_map([0, 4, 6], [nan] * 3, 7), ins=Insert(20, nan, feats_on([100, 150])), window=3, th=0.2, victim_row=0)
    c["all_nan_without_key_frame_0"] = dict(m=small_map([2, 4, 6], [nan] * 3, 7), ins=Insert(20, nan, feats_on([100, 150])), window=3, th=0.2, status=INVALID)
    # scan and chunk edges of the 512-thread workgroup
    for n_obs in (0, 1, 511, 512, 513, 1025):
        c["obs_%d" % n_obs] = sized_case(max(1, n_obs // 3), n_obs, 40, 0x100 + n_obs)
    for n_feat in (0, 1, 64, 65, 511, 512, 513):
        c["feat_%d" % n_feat] = sized_case(100, 300, n_feat, 0x200 + n_feat)
    for n_mp in (1, 511, 512, 513):
        c["mp_%d" % n_mp] = sized_case(n_mp, 2 * n_mp + 1, 70, 0x300 + n_mp)
    return c
