"""The mapper's rules on the CPU (tests/mapper_ref.py): the gate against its written table, and the call as a walk composed of the existing walks, run
over the histories of tests/whole_map_model.py in banks of six with a seeded idle pattern between an item's key-frames.  After every call the walk's
tables, map archive and prior rows must be the object model's; an idle call must change no byte; a refused key-frame in the buffers is kept out by the
turn's status alone; the history that ends on the archive's caps faults, and the fault sticks.  The oracle's solve supplies the numbers, as in
tests/test_whole_map_model.py.  CPU only."""
import numpy as np
import pytest

import backend_ref as br
import map_archive_ref as mr
import mapper_ref as mp
import obs_archive_ref as oa
import test_whole_map_model as T
import whole_map_model as wm

BANKS = (T.HISTORIES[:6], T.HISTORIES[6:])
PATTERN_SEED = 5         # chosen so that every history reaches its last key-frame and every item idles between two of its key-frames (asserted below)
_SCRIPTS = {}


def script(pkg, oracle, spec):
    """[(the corrections before it, the Entry, the model after it)] of one history, computed once"""
    if spec not in _SCRIPTS:
        m = wm.WholeMap(pkg.chain, spec[1])
        out, corr = [], []
        for e in mp.drive(pkg, oracle, spec, m):
            if e.kind == "correct":
                corr.append(e)
            else:
                out.append((corr, e, m.clone()))
                corr = []
        _SCRIPTS[spec] = out
    return _SCRIPTS[spec]


def test_gate_table():
    assert len(mp.GATE_TABLE) == 16 and len({r[:3] for r in mp.GATE_TABLE}) == 16
    assert {r[0] for r in mp.GATE_TABLE} == {0, mp.NO_TURN, mp.INIT_RETRY, mp.ERR_CAPACITY} and {r[1] >= 0 for r in mp.GATE_TABLE} == {True, False}
    for status, kf_id, fault, want in mp.GATE_TABLE:
        assert mp.gate(status, kf_id, fault) == want, (status, kf_id, fault)
    assert [r[3] for r in mp.GATE_TABLE].count(0) == 1 and mp.IDLE not in (0, mp.NO_TURN, mp.INIT_RETRY) and mp.IDLE > 0


def apply_corrections(it, corr):
    for c in corr:                                                          # what the corrector's write-back does: rows found by id
        for k in it.w.kfs:
            it.w.kfs[k] = c.kf_pose[k].copy()
        for i, p in it.w.mps.items():
            p.pos = c.mp_pos[i].copy()
        for r, k in enumerate(it.a.kf_id):
            it.a.kf_pose[r] = c.kf_pose[k].copy()
        for s, i in enumerate(it.a.mp_id):
            if i in c.mp_pos:
                it.a.mp_pos[s] = c.mp_pos[i].copy()


@pytest.mark.parametrize("n", range(len(BANKS)))
def test_walk_equals_the_model_under_the_idle_pattern(pkg, oracle, n):
    specs, chain = BANKS[n], pkg.chain
    scripts = [script(pkg, oracle, s) for s in specs]
    solve = T.oracle_solve(oracle)
    items = [mp.Item() for _ in specs]
    at, idles, last_ins, model = [0] * 6, [0] * 6, [None] * 6, [None] * 6
    idle_between = [0] * 6                                                  # idle calls after the item's first key-frame and before its last
    seen = dict(all_idle=0, all_take=0, mixed=0, refused=0, capacity=0, empty=0, stale_idle=0, takes=0)
    last_take = [max(i for i, (_, e, _) in enumerate(sc) if e.kind == "take") for sc in scripts]
    for take in mp.rounds(6, [len(s) for s in scripts], PATTERN_SEED):
        kinds = []
        for b, it in enumerate(items):
            before, fault = it.bytes(), it.fault
            dist = lambda pk, pn, row: wm.WholeMap.dist(model[b] or scripts[b][0][2], pk, pn)
            if take[b]:
                corr, e, m = scripts[b][at[b]]
                at[b] += 1
                apply_corrections(it, corr)
                if e.kind == "take":
                    words, rep = mp.call(chain, it, 0, e.ins, specs[b][1], solve, dist)
                    done = e.opt_status == br.DONE
                    assert words == [0, 0, 0, mr.UPDATED, oa.UPDATED, e.opt_status] + [mr.UPDATED if done else mr.SKIPPED] * 2, (specs[b], at[b], words)
                    assert oa.same_priors(rep["priors"], e.ins.priors), (specs[b], at[b])      # the store's rows are the model's GetObservations()
                    assert T.same_tables(br.pack(it.w), br.pack(m.active_map())) is None, (specs[b], at[b])
                    assert mr.check_against_chain(it.a, m, m.erased) is None, (specs[b], at[b], mr.check_against_chain(it.a, m, m.erased))
                    model[b], last_ins[b] = m, e.ins
                    seen["takes"] += 1; seen["empty"] += not done
                    kinds.append("take")
                    continue
                if e.kind == "capacity":                                    # the archive's caps are met exactly: this key-frame is one too many
                    caps = (len(it.a.kf_id), len(it.a.edge_v0), len(it.a.mp_id))
                    arch = it.a.arrays()
                    words, _ = mp.call(chain, it, 0, e.ins, specs[b][1], solve, dist, arch_caps=caps)
                    assert words[0] == words[3] == mp.ERR_CAPACITY and words[1:3] == [0, 0] and it.fault == mp.ERR_CAPACITY, words
                    assert mr.same(arch, it.a.arrays()) is None
                    seen["capacity"] += 1
                    kinds.append("take")
                    continue
                assert e.kind == "refused"                                  # a key-frame in the buffers, id and features valid, under a turn status 1
                words, _ = mp.call(chain, it, mp.NO_TURN, e.ins, specs[b][1], solve, dist)
                seen["refused"] += 1
            else:
                status, ins = mp.idle_buffers(idles[b], last_ins[b])
                seen["stale_idle"] += ins is not None
                idles[b] += 1
                idle_between[b] += 0 < at[b] <= last_take[b]
                words, _ = mp.call(chain, it, status, ins, specs[b][1], solve, dist)
            kinds.append("idle")
            assert words == [fault if fault else mp.IDLE] + [mp.IDLE] * 7, (specs[b], words)
            assert it.bytes() == before and it.fault == fault, specs[b]
        seen["all_idle"] += all(k == "idle" for k in kinds); seen["all_take"] += all(k == "take" for k in kinds)
        seen["mixed"] += len(set(kinds)) == 2
    print("bank %d:" % n, seen, "idle calls per item", idles, "between key-frames", idle_between)
    for b, (it, spec) in enumerate(zip(items, specs)):                      # the condition: every history reached its last key-frame
        assert at[b] == len(scripts[b]) and len(model[b].all_kfs) == spec[2] and len(it.a.kf_id) == spec[2], (spec, at[b])
        assert idles[b] >= 2 and idle_between[b] >= 2, (spec, idles[b], idle_between[b])
        if "capacity" in spec[4]:                                           # the closing idle calls reported the fault, and nothing moved
            assert it.fault == mp.ERR_CAPACITY
    assert seen["all_idle"] >= 1 and seen["all_take"] >= 1 and seen["mixed"] >= 8 and seen["stale_idle"] >= 6
    assert seen["capacity"] == sum("capacity" in s[4] for s in specs) and seen["refused"] >= sum("refused" in s[4] for s in specs)
    assert seen["empty"] >= sum("empty" in s[4] for s in specs)


def test_a_refused_insert_faults_the_item_and_is_not_optimised(pkg, oracle):
    """the key-frame id is not above the table's last: the insert answers ERR_INVALID, the flatten is gated on that status, the fault sticks"""
    spec = T.HISTORIES[5]
    sc = script(pkg, oracle, spec)
    it, solve = mp.Item(), T.oracle_solve(oracle)
    dist = lambda pk, pn, row: wm.WholeMap.dist(sc[0][2], pk, pn)
    for corr, e, m in sc[:3]:
        assert e.kind == "take"
        apply_corrections(it, corr)
        assert mp.call(pkg.chain, it, 0, e.ins, spec[1], solve, dist)[0][0] == 0
    before = it.bytes()
    words, _ = mp.call(pkg.chain, it, 0, sc[1][1].ins, spec[1], solve, dist)            # key-frame 2 once more
    assert words == [mp.ERR_INVALID, 0, mp.ERR_INVALID, mr.SKIPPED, oa.SKIPPED, mp.IDLE, mr.SKIPPED, oa.SKIPPED] and it.bytes() == before
    for e in (sc[3][1], sc[4][1]):                                          # the stream's later key-frames: kept out, the same error
        words, _ = mp.call(pkg.chain, it, 0, e.ins, spec[1], solve, dist)
        assert words == [mp.ERR_INVALID] + [mp.IDLE] * 7 and it.bytes() == before
    fresh = mp.Item()                                                       # what myslam_mapper_reset_item leaves: an empty item is served again
    assert mp.call(pkg.chain, fresh, 0, sc[0][1].ins, spec[1], solve, dist)[0][0] == 0
