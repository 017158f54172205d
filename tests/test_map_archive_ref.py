"""The rules of myslam_map_update_batch (include/myslam_hip.h) as tests/map_archive_ref.py walks them, pinned against <pkg>/chain.py: the 44-frame
rendered run of tests/test_chain_host.py through Chain(OracleBackend) with a window of 3 key-frames, the walk fed what the back end's tables, reports
and outlier lists would hold after every Map::InsertKeyFrame and every Backend::OptimizeActiveMap.  At every key-frame the walk's archive must be
Chain's all_kfs / all_mps / last_kf.  Then the checker is rehearsed on four faulty stand-ins.  CPU only.

meas against Chain's rel_to_last: the host turn stores cur.rel itself, the archive recomputes T(new) * T(prev)^-1 from the two stored poses.  Measured
on this run (printed by the test, no bar set): at most 1.33e-15 in any component over the 40 edges; DESIGN.md section 3.16c.

The first-observer rule that is pinned here is the header's (window record, mp_gone_kf).  The shorter rule "the record stays when the front row has
obs_kf = -1" fails this pin at map point 352, key-frame 29: BA removes its front observation and the next one belongs to a key-frame that left.
That is ONE witness in this run.  The rule is pinned a second time in tests/test_whole_map_model.py: 12 seeded random histories on an object model of
the reference's Map (tests/whole_map_model.py), where that case occurs 34 times, the front removed with the next observer in the window 35 times, and
where the shorter rule and "the last instead of the lowest departed observer" are rehearsed as stand-ins of their own (map_archive_ref.MORE_FAULTS);
test_path_counters there prints the counts.  The rendered run stays the only pin against <pkg>/chain.py's own objects."""
import numpy as np
import pytest

import map_archive_ref as mr
from oracle_backend import OracleBackend


# trackingGood 390 (tests/test_chain_host.py) never lets BA remove a front observation within 44 frames at any window from 2 to 7; 400 makes 41
# key-frames, one such removal, 91 points erased by BA, 78 that left alive and 67 outlier-list points erased while not active
CFG = {"numFeatures.trackingGood": 400, "Map.activeMap.size": 3}


class _Refused(Exception):
    pass


def _run(pkg, synth, oracle, faults=(), cfg=None):
    """-> (first mismatch or None, facts about the run, the walk's archive, the Chain)"""
    chain = pkg.chain
    scene = synth.sequence_scene(); C, yaw = synth.sequence_poses(200)
    frames = [synth.render_stereo(scene, C[t], yaw[t], t) for t in range(44)]
    cfg = dict(cfg or CFG)
    a = mr.Archive()
    facts = dict(erased_by_ba=0, left_alive=0, front_removed=0, promoted=0, empty=0, checks=0, dev=[])
    bad, erased, meas_inputs = [], set(), {}

    class Pinned(chain.Chain):
        def remove_all_outlier_map_points(self):
            erased.update(m for m in self.outlier_mps if m in self.all_mps)
            super().remove_all_outlier_map_points()

        def remove_map_point(self, mp):
            erased.add(mp.id)
            super().remove_map_point(mp)

        def map_insert_keyframe(self, kf):
            outl = list(self.outlier_mps)
            if kf.last_kf is not None:              # the two poses the formula reads, as Chain holds them when the key-frame is inserted
                meas_inputs[kf.id] = (np.array(kf.pose, float), np.array(kf.last_kf.pose, float))
            before = set(self.active_mps)
            super().map_insert_keyframe(kf)
            facts["left_alive"] += sum(1 for m in before if m not in self.active_mps and m in self.all_mps)      # RemoveOldActiveMapPoints
            st = mr.update(chain, a, mr.AFTER_INSERT, mr.pack_chain(self), 0, outlier_ids=outl, faults=faults)
            assert st == mr.UPDATED, st
            self._check("insert of key-frame %d" % kf.id)

        def optimize_active_map(self):
            before = sorted(self.active_mps)
            first = {m: (self.active_mps[m].obs[0] if self.active_mps[m].obs else None) for m in before}
            listed = [m for m in self.outlier_mps if m not in self.active_mps and m in self.all_mps]
            n_ba = sum(1 for t, _ in self.log if t == "ba")
            super().optimize_active_map()
            ran = sum(1 for t, _ in self.log if t == "ba") > n_ba
            rep = np.array([(2 if m not in self.all_mps else (1 if m not in self.active_mps else 0)) for m in before], np.uint8)
            if ran:
                facts["erased_by_ba"] += int((rep == 2).sum()); facts["left_alive"] += int((rep == 1).sum()); facts["promoted"] += len(listed)
                facts["front_removed"] += sum(1 for m in before if m in self.all_mps and first[m] is not None and self.all_mps[m].obs
                                              and self.all_mps[m].obs[0] is not first[m])
            else:
                facts["empty"] += 1
            st = mr.update(chain, a, mr.AFTER_OPTIMIZE, mr.pack_chain(self), 0 if ran else 1, mp_report=rep, faults=faults)
            assert st == (mr.UPDATED if ran else mr.SKIPPED), st
            self._check("optimise after key-frame %d" % max(self.all_kfs))

        def _check(self, where):
            facts["checks"] += 1
            why = mr.check_against_chain(a, self, erased)
            if why is not None:
                bad.append((where, why))
                if faults:                          # a stand-in is refused at its first mismatch: no need to finish the run
                    raise _Refused()

    try:
        c = Pinned(OracleBackend(oracle, synth.calc_weights_handcrafted(), cfg, chain), pkg.api, synth.SEQ_K, frames, cfg=cfg).run()
    except _Refused:
        return bad[0], facts, a, None
    kfs = sorted(c.all_kfs)
    for e, (v0, v1) in enumerate(zip(a.edge_v0, a.edge_v1)):
        facts["dev"].append(float(np.abs(np.asarray(a.meas[e]) - np.asarray(c.all_kfs[kfs[v0]].rel_to_last)).max()))
    facts["meas_inputs"] = meas_inputs
    return (bad[0] if bad else None), facts, a, c


@pytest.fixture(scope="module")
def pinned(pkg, synth, oracle):
    return _run(pkg, synth, oracle)


def test_walk_equals_chain_at_every_keyframe(pinned):
    bad, facts, a, c = pinned
    print("run facts:", {k: v for k, v in facts.items() if k not in ("dev", "meas_inputs")})
    assert bad is None, bad
    assert len(a.kf_id) >= 8 and facts["checks"] >= 2 * len(a.kf_id) - 1 and len(c.active_kfs) == 3
    # the run holds every path the rules name: a point erased by BA, a point that left alive, a front observation removed by BA
    assert facts["erased_by_ba"] >= 1 and facts["left_alive"] >= 1 and facts["front_removed"] >= 1, facts
    assert len(a.edge_v0) == len(a.kf_id) - 1 and 2 in a.mp_state and 0 in a.mp_state


def test_meas_is_the_stated_formula_bit_for_bit(pinned, pkg):
    _, facts, a, c = pinned
    chain = pkg.chain
    kfs = sorted(c.all_kfs)
    # the archive's previous pose at the insert is Chain's pose of last_kf when the new key-frame was made
    assert len(a.meas) >= 7
    for e, (v0, v1) in enumerate(zip(a.edge_v0, a.edge_v1)):
        new, prev = facts["meas_inputs"][kfs[v0]]
        assert v1 == v0 - 1 and np.asarray(a.meas[e]).tobytes() == mr.edge_meas(chain, new, prev).tobytes()
    print("max |meas - rel_to_last| per edge:", ["%.3g" % d for d in facts["dev"]], "max %.3g" % max(facts["dev"]))


@pytest.mark.parametrize("fault", mr.FAULTS)
def test_checker_refuses_faulty_stand_ins(fault, pkg, synth, oracle):
    bad, _, _, _ = _run(pkg, synth, oracle, faults=(fault,))
    assert bad is not None, fault
    print(fault, "->", bad)
