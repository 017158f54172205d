"""myslam_mapper_keyframe_batch (include/myslam_hip.h, MAPPER) in plain Python: the gate as a function with its written table, and one call of one item as
a walk that composes the existing walks (obs_archive_ref.prior_rows, map_insert_ref.insert_walk, map_archive_ref.update, obs_archive_ref.update,
backend_ref.walk) behind that gate, with the sticky fault.  Also what the CPU and the GPU test share: the histories of tests/whole_map_model.py driven on
the object model with the oracle's solve (drive), and the seeded idle pattern laid between an item's key-frames (rounds).  Test helper, no GPU."""
import numpy as np

import backend_ref as br
import map_archive_ref as mr
import map_insert_ref as mi
import obs_archive_ref as oa
import whole_map_model as wm

IDLE, STATUS_WORDS = 3, 8                                   # MYSLAM_MAPPER_IDLE, MYSLAM_MAPPER_STATUS_WORDS
NO_TURN, INIT_RETRY, ERR_INVALID, ERR_CAPACITY = 1, 2, -1, -3   # MYSLAM_TRACKER_NO_TURN / _INIT_RETRY, MYSLAM_ERR_*
K = (718.856, 718.856, 607.1928, 185.2157)


def gate(report_status, new_kf_id, fault):
    """k_mapper_gate: 0 = the item takes the key-frame, else IDLE"""
    return 0 if (fault == 0 and report_status == 0 and new_kf_id >= 0) else IDLE


# (turn status d_report[s][0], d_new_kf_id[s], sticky fault) -> the gate.  Written out, not computed: every combination of the four statuses a turn
# or an init can leave, an id or none, a fault or none.  Only the first row takes the key-frame.
GATE_TABLE = (
    (0, 7, 0, 0),
    (0, 7, ERR_CAPACITY, IDLE),
    (0, -1, 0, IDLE),
    (0, -1, ERR_CAPACITY, IDLE),
    (NO_TURN, 7, 0, IDLE),
    (NO_TURN, 7, ERR_INVALID, IDLE),
    (NO_TURN, -1, 0, IDLE),
    (NO_TURN, -1, ERR_INVALID, IDLE),
    (INIT_RETRY, 7, 0, IDLE),
    (INIT_RETRY, 7, ERR_CAPACITY, IDLE),
    (INIT_RETRY, -1, 0, IDLE),
    (INIT_RETRY, -1, ERR_CAPACITY, IDLE),
    (ERR_CAPACITY, 7, 0, IDLE),
    (ERR_CAPACITY, 7, ERR_INVALID, IDLE),
    (ERR_CAPACITY, -1, 0, IDLE),
    (ERR_CAPACITY, -1, ERR_INVALID, IDLE),
)


class Item:
    """one stream's state behind the handle: the back end's tables (a backend_ref.Map), the map archive, the observation archive, the sticky fault"""

    def __init__(self, row_cap=1 << 20):
        self.w, self.a, self.o, self.fault = br.Map(), mr.Archive(), oa.Store(row_cap), 0

    def bytes(self):
        """every byte the three units hold of the item, for 'an idle call changes nothing'"""
        t, a, o = br.pack(self.w), self.a.arrays(), self.o.arrays(self.a)
        parts = [np.ascontiguousarray(t[k]).tobytes() for k in sorted(t)] + [np.ascontiguousarray(a[k]).tobytes() for k in sorted(a)]
        parts += [np.ascontiguousarray(o[k]).tobytes() for k in oa.GET_FIELDS] + [bytes([o["rows_in_use"] & 255, o["n_reclaims"] & 255, o["error"] & 255])]
        return b"|".join(parts)


def call(chain, it, report_status, ins, window, solve, dist, be_caps=None, arch_caps=None, prior_cap=1 << 20, min_dis_th=0.2):
    """One item of one myslam_mapper_keyframe_batch.  ins: the map_insert_ref.Insert in the turn's buffers (priors are not read: they come from the
    item's own store), None = id -1 and no feature.  -> (the 8 status words, the reports of the stages that ran)"""
    new_id = ins.kf_id if ins is not None else -1
    if gate(report_status, new_id, it.fault) != 0:
        return [it.fault if it.fault else IDLE] + [IDLE] * 7, {}
    st = [0] * 7
    st[0], priors = oa.prior_rows(it.o, [f[0] for f in ins.feats], br.pack(it.w)["mp_id"], it.a, prior_cap)
    ins2 = mi.Insert(ins.kf_id, ins.kf_pose, ins.feats, priors, ins.outlier_ids)
    ri = mi.insert_walk(it.w, ins2, window, min_dis_th, dist, caps=be_caps)
    st[1] = ri["status"]
    st[2] = mr.update(chain, it.a, mr.AFTER_INSERT, br.pack(it.w), st[1], outlier_ids=ins.outlier_ids, caps=arch_caps)
    st[3] = oa.update(it.o, oa.AFTER_INSERT, br.pack(it.w), st[1], st[2], it.a)
    ro = None
    if st[1] != 0:                                          # the flatten is gated on the insert's status: a refused key-frame is not optimised
        st[4] = IDLE
    else:
        ro = br.walk(it.w, solve)
        st[4] = ro["status"]
    t = br.pack(it.w)
    st[5] = mr.update(chain, it.a, mr.AFTER_OPTIMIZE, t, st[4], mp_report=ro["mp_report"] if ro else None, caps=arch_caps,
                      left_pos=ro["left_pos"] if ro else None)
    st[6] = oa.update(it.o, oa.AFTER_OPTIMIZE, t, st[4], st[5], it.a, obs_report=ro["obs_report"] if ro else None)
    overall = next((v for v in st if v < 0), 0)
    if overall < 0:
        it.fault = overall
    return [overall] + st, dict(priors=priors, insert=ri, optimize=ro)


class Entry:
    """one thing that happens to a stream: kind "take" (a key-frame: insert + optimise), "refused" (the turn's buffers hold a key-frame the stream must
    not take: served as an idle call), "capacity" (a key-frame the archive's caps refuse: the stream's last), "correct" (poses / positions moved from
    outside between two calls: kf_pose / mp_pos = every value of the model afterwards, by id)"""

    def __init__(self, kind, ins=None, kf_pose=None, mp_pos=None, opt_status=None, n_flags=0):
        self.kind, self.ins, self.kf_pose, self.mp_pos, self.opt_status, self.n_flags = kind, ins, kf_pose, mp_pos, opt_status, n_flags


def drive(pkg, oracle, spec, m=None):
    """The history `spec` (tests/test_whole_map_model.HISTORIES) on the object model, the oracle's solve supplying the numbers of every optimise: yields an
    Entry AFTER the model has taken it.  Unlike the hand-wired chain the model optimises only after a key-frame (src/backend.cpp:30-37): the idle
    optimise that follows a refused insert in the history is dropped.  m: the caller's WholeMap (to look at after every entry)."""
    seed, window, n_kf, n_steps, extras = spec
    m = m if m is not None else wm.WholeMap(pkg.chain, window)
    gen = wm.history(seed, m, K, n_kf, n_steps, extras)
    for ev in gen:
        if ev.kind == "correct":
            m.correct(ev.rigid, ev.moves)
            yield Entry("correct", kf_pose={k: kf.pose.copy() for k, kf in m.all_kfs.items()}, mp_pos={i: mp.pos.copy() for i, mp in m.all_mps.items()})
        elif ev.kind == "refused":
            nxt = next(gen)
            assert nxt.kind == "optimize" and not nxt.flags
            yield Entry("refused", ins=ev.ins)
        elif ev.kind == "capacity":
            yield Entry("capacity", ins=ev.ins)
            return
        else:
            assert ev.kind == "insert"
            rm = m.insert_keyframe(ev.ins)
            assert rm["status"] == mi.OK and (not rm["branch"] or wm.margins_ok(rm, 0.2, wm.MARGIN))
            opt = next(gen)
            assert opt.kind == "optimize"
            flat, edge_objs, slot_mps = br.flatten(m.active_map())
            sol = {}

            def poses():
                p2, x2, chi, out, _, _ = oracle.ba_optimize_active_map(np.stack([m.active_kfs[k].pose for k in sorted(m.active_kfs)]),
                                                                       np.stack([mp.pos for mp in slot_mps]), flat["edge_pose"], flat["edge_pt"],
                                                                       flat["edge_obs"], flat["fixed"], K)
                want = np.array([o.tag in opt.flags for _, o in edge_objs])
                # the precondition of the constructed flags: the solve flags exactly them, and no chi2 is anywhere near the threshold
                assert np.array_equal(out.astype(bool), want) and (chi[~want] < 1.0).all() and (chi[want] > 50.0).all(), spec
                sol["x"] = {mp.id: x2[j] for j, mp in enumerate(slot_mps)}
                return {k: p2[i] for i, k in enumerate(sorted(m.active_kfs))}

            ro = m.optimize(opt.flags, poses, lambda: sol["x"])
            yield Entry("take", ins=ev.ins, opt_status=ro["status"], n_flags=len(opt.flags))


def rounds(n_items, lengths, seed):
    """The idle pattern: for every call of a bank, which items take their next entry (True) and which idle.  Call 0: every item takes (every history
    opens with a key-frame); call 2: every item idles, between its first key-frame and the rest; otherwise an item idles with probability 0.3.  When
    every item has used its `lengths[b]` entries two calls follow in which every item idles, so each item idles three times at least."""
    rng = np.random.default_rng([int(seed), 0x1D1E])
    left = list(lengths)
    idled = [0] * n_items
    n = 0
    while any(left):
        if n == 0:
            take = [True] * n_items
        elif n == 2:
            take = [False] * n_items
        else:
            take = [bool(left[b]) and (rng.random() >= 0.3) for b in range(n_items)]
            if not any(take):                                # never a second all-idle call by accident: the longest history moves on
                take[int(np.argmax(left))] = True
        for b in range(n_items):
            if take[b] and left[b]:
                left[b] -= 1
            else:
                take[b] = False
                idled[b] += 1
        yield take
        n += 1
    for _ in range(2):                                      # two closing calls in which every item idles: a finished stream, a faulted one
        yield [False] * n_items


def idle_buffers(n, last_ins):
    """What the turn's buffers hold for an item without a key-frame, three kinds in rotation -> (turn status, Insert or None): not eligible (id -1, no
    feature), an init that must retry (the same), a turn refused for capacity whose rows are unspecified — here the stream's previous key-frame whole,
    id included, so only the status keeps it out."""
    kind = n % 3
    if kind == 2 and last_ins is not None:
        return ERR_CAPACITY, last_ins
    return (NO_TURN, INIT_RETRY, NO_TURN)[kind], None
